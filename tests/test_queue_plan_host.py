"""CPU suite: the queue plan's host logic (csrc/queue_plan.h).  The classification of candidate
streams and the choice among them are driven by tools/queue_plan_check.cpp with a fake runtime; nothing of it is loaded
into Python and no call touches a GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_exported_and_declared(pkg):
    lib = pkg.load_library()
    text = open(pkg.INCLUDE).read()
    assert hasattr(lib, "nblic_amd_queue_plan_stats") and "nblic_amd_queue_plan_stats" in pkg.EXPORTS
    assert re.search(r"\bnblic_amd_queue_plan_stats\s*\(", text)
    assert lib.nblic_amd_queue_plan_stats(None, None, None) == -1


def test_no_hip_in_the_interface():
    """queue_plan.h is host-only: it compiles without the HIP headers (the stand-alone check does just that) and names
    no HIP type or call."""
    text = open(os.path.join(ROOT, "nblic-image-compression_amd", "csrc", "queue_plan.h")).read()
    assert "#include <hip" not in text and not re.search(r"\bhip[A-Z]\w*\b", text)


def test_the_library_names_no_runtime_queue_switch():
    """The library neither sets nor reads the runtime's queue count or any other queue switch of the runtime, and asks for
    no stream priorities: the plan works with the queues the process has."""
    csrc = os.path.join(ROOT, "nblic-image-compression_amd", "csrc")
    for name in ("queue_plan.h", "pipeline.hip", "hip_owned.h"):
        text = open(os.path.join(csrc, name)).read()
        assert "GPU_MAX_HW_QUEUES" not in text and "hipStreamCreateWithPriority" not in text, name
        assert not re.search(r"(setenv|putenv)\s*\(", text), name


def test_standalone_check_under_sanitizers(tmp_path):
    """tools/queue_plan_check.cpp: queue_plan.h alone, with its own main, under the address and undefined-behaviour
    sanitizers: 3, 4, 6 and 12 groups over round-robin dealing to 1-16 queues, least-loaded dealing with 0-3 streams held
    on one queue beforehand (six groups on four queues come out 2 / 2 / 1 / 1), the runtime with one queue, an error at
    every call in turn, the candidate cap reached before balance."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "queue_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread", "-o", exe,
                    os.path.join(ROOT, "tools", "queue_plan_check.cpp"), "-ldl"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert "queue_plan_check ok" in r.stdout
