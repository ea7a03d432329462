"""GPU suite (-m gpu): the queue plan of a context with three groups or more (csrc/queue_plan.h).
Six groups of two slots encode 24 SYN-1 frames of 64 x 64 -- every group launches twice and more, each on the stream the
plan handed it -- with the plan on and with NBLIC_AMD_QUEUE_PLAN=0, a fresh process per setting because the switch is read
when the context is created.  This is the smallest shape at which a wrong hand-over of streams could still show: a group
launching on a destroyed candidate, or two groups sharing one stream.  Which queues the streams sit on is the machine's
business and is not asserted; profiles/r29_queue_occupancy_after.json is the record of that."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES, H, W, GROUPS, GROUP_SIZE = 24, 64, 64, 6, 2

_CHILD = (
    "import importlib, json, sys\n"
    "sys.path.insert(0, %r)\n"
    "import torch; torch.cuda.init()\n"
    "pkg = importlib.import_module('nblic-image-compression_amd')\n"
    "imgs = [pkg.syn1(%d, %d, 1 + k) for k in range(%d)]\n"
    "ctx = pkg.Context(0, n_slots=%d, n_coders=2, n_groups=%d)\n"
    "got = ctx.encode_batch(imgs)\n"
    "plan = ctx.queue_plan()\n"
    "ctx.close()\n"
    "print('RESULT ' + json.dumps({'streams': [g.hex() for g in got], 'plan': plan, 'live': pkg.live_resources()}))\n"
)


def _child(env_extra):
    code = _CHILD % (ROOT, H, W, FRAMES, GROUPS * GROUP_SIZE, GROUPS)
    env = dict(os.environ, **env_extra)
    if not env_extra:
        env.pop("NBLIC_AMD_QUEUE_PLAN", None)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):]), r.stderr


@pytest.fixture(scope="module")
def want(pkg, oracle, gpu_ctx):                                  # (gpu_ctx first: torch initialises its runtime before the library is loaded)
    return [oracle.encode(pkg.syn1(H, W, 1 + k), 0, 1)[0] for k in range(FRAMES)]


@pytest.fixture(scope="module")
def runs():
    return {"on": _child({}), "off": _child({"NBLIC_AMD_QUEUE_PLAN": "0"})}


def test_streams_with_the_plan_on_and_off(want, runs):
    on, off = runs["on"][0], runs["off"][0]
    print("plan on:", on["plan"], "off:", off["plan"])
    for k, w in enumerate(want):
        assert bytes.fromhex(on["streams"][k]) == w, (k, "plan on")
        assert bytes.fromhex(off["streams"][k]) == w, (k, "plan off")
    assert on["streams"] == off["streams"]
    for r in (on, off):                                         # a process that had this one context only holds nothing after close()
        assert all(v == 0 for v in r["live"].values()), r["live"]


def test_stats_are_self_consistent(runs):
    plan, err = runs["on"]
    plan = plan["plan"]
    print(plan, err.strip())
    assert plan["n_groups"] == GROUPS
    assert plan["classes"] >= 1
    assert len(plan["groups_per_class"]) == plan["classes"] and sum(plan["groups_per_class"]) == GROUPS
    assert plan["state"] in ("on", "one_class")                  # (one class: a process with a single hardware queue)
    assert plan["on"] == (plan["state"] == "on")
    if plan["on"]:
        assert max(plan["groups_per_class"]) - min(plan["groups_per_class"]) <= 1
        assert plan["spread"] == max(plan["groups_per_class"]) - min(plan["groups_per_class"]) <= plan["unplanned_spread"]
        assert GROUPS <= plan["candidates"] <= 4 * GROUPS
        assert "queue plan off" not in err
    else:
        assert "queue plan off" in err                           # one line says why
    assert plan["plan_ms"] > 0.0                                 # the plan ran, and what it cost is reported


def test_the_switch(runs):
    plan, err = runs["off"]
    plan = plan["plan"]
    assert plan["state"] == "switched_off" and not plan["on"]
    assert plan["candidates"] == 0 and plan["classes"] == 0 and plan["plan_ms"] == 0.0
    assert err.count("queue plan off") == 1


def test_two_groups_pay_nothing(gpu_ctx):
    plan = gpu_ctx.queue_plan()
    assert plan["state"] == "few_groups" and not plan["on"]
    assert plan["candidates"] == 0 and plan["classes"] == 0 and plan["plan_ms"] == 0.0 and plan["groups_per_class"] == []


def test_no_candidate_leaks(pkg, gpu_ctx):
    """Ten contexts of six groups created and destroyed: the library holds what it held before, so every candidate stream
    the plan created was either handed to a group or destroyed."""
    before = pkg.live_resources()
    for _ in range(10):
        ctx = pkg.Context(0, n_slots=GROUPS, n_coders=1, n_groups=GROUPS)
        try:
            assert ctx.queue_plan()["n_groups"] == GROUPS
        finally:
            ctx.close()
    assert pkg.live_resources() == before
