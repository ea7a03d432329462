#!/usr/bin/env python3
"""Per hardware queue: how long it was busy and with which kernels, from one rocprofv3 --kernel-trace run of bench.py.

    python tools/queue_occupancy.py TRACE_DIR --steps 3 [--bench-json FILE] [--note TEXT] > profiles/rNN_queue_occupancy.json

TRACE_DIR is searched for *_kernel_trace.csv (CSV output) or *_results.db (rocpd output).  --steps is the number of
bench steps the trace holds, warm-up included: the per-step figures are the totals divided by it.  A queue's busy time
is the union of its kernels' [start, end] intervals; `sum_ms` is their plain sum (larger where kernels of one queue
overlap).  The runtime's copy kernels are the ones whose name holds `copyBuffer` (the blit kernels of hipMemcpyAsync).
"""
import argparse
import collections
import csv
import glob
import json
import os
import re
import sqlite3


def short(name):
    """void nblic::k_mix<true>(Args...) [clone .kd] -> k_mix"""
    name = re.sub(r"\s*\[clone.*$", "", name).replace(".kd", "")
    m = re.match(r"^(?:void\s+)?([A-Za-z_][\w:]*)", name)
    return m.group(1).split("::")[-1] if m else name


def rows_of(trace_dir):
    """(queue id, kernel name, start ns, end ns) of every dispatch."""
    out = []
    for f in glob.glob(os.path.join(trace_dir, "**", "*_kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            out.append((str(r["Queue_Id"]), r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    if out:
        return out
    for f in glob.glob(os.path.join(trace_dir, "**", "*_results.db"), recursive=True):
        db = sqlite3.connect(f)
        cols = [c[1] for c in db.execute("pragma table_info(kernels)")]
        pick = lambda *names: next(n for n in names if n in cols)
        q = "select %s, %s, %s, %s from kernels" % (pick("queue_id", "queue"), pick("name", "kernel_name"), pick("start", "start_timestamp"), pick("end", "end_timestamp"))
        out += [(str(a), b, int(c), int(d)) for a, b, c, d in db.execute(q)]
    return out


def union_ns(intervals):
    busy, cur_s, cur_e = 0, None, None
    for s, e in sorted(intervals):
        if cur_e is None or s > cur_e:
            if cur_e is not None:
                busy += cur_e - cur_s
            cur_s, cur_e = s, e
        else:
            cur_e = max(cur_e, e)
    return busy + (cur_e - cur_s if cur_e is not None else 0)


def summarize(rows, steps):
    t0, t1 = min(r[2] for r in rows), max(r[3] for r in rows)
    by_q = collections.defaultdict(list)
    for q, name, s, e in rows:
        by_q[q].append((short(name), s, e))
    ms = lambda ns: round(ns / 1e6, 2)
    queues = {}
    for q, ks in sorted(by_q.items()):
        split = collections.defaultdict(lambda: [0, 0])
        for name, s, e in ks:
            split[name][0] += 1
            split[name][1] += e - s
        queues[q] = {"busy_ms": ms(union_ns([(s, e) for _, s, e in ks])), "sum_ms": ms(sum(e - s for _, s, e in ks)), "dispatches": len(ks),
                     "by_kernel": {n: {"dispatches": c, "sum_ms": ms(t)} for n, (c, t) in sorted(split.items(), key=lambda kv: -kv[1][1])}}
    per_step = collections.defaultdict(int)
    for _, name, _, _ in rows:
        per_step[short(name)] += 1
    copies = sum(c for n, c in per_step.items() if "copyBuffer" in n)
    return {"steps_in_trace": steps, "span_ms": ms(t1 - t0), "hardware_queues": len(queues), "all_queues_busy_union_ms": ms(union_ns([(s, e) for _, _, s, e in rows])),
            "dispatches_per_step": {"runtime_copy_kernels": round(copies / steps, 1), "all": round(len(rows) / steps, 1),
                                    "by_kernel": {n: round(c / steps, 1) for n, c in sorted(per_step.items(), key=lambda kv: -kv[1])}},
            "queues": queues}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace_dir")
    ap.add_argument("--steps", type=int, required=True)
    ap.add_argument("--bench-json", default=None, help="the bench line printed by the traced run: its value and toggles are copied into the record")
    ap.add_argument("--note", default=None, help="a line kept with the record: which library and settings the traced run had")
    a = ap.parse_args()
    rows = rows_of(a.trace_dir)
    if not rows:
        raise SystemExit("no kernel trace under " + a.trace_dir)
    rec = summarize(rows, a.steps)
    if a.bench_json and os.path.exists(a.bench_json):
        lines = [l for l in open(a.bench_json).read().splitlines() if l.startswith("{")]
        if lines:
            d = json.loads(lines[-1])
            rec["traced_bench"] = {k: d.get(k) for k in ("value", "unit", "host_coder_Mbins_per_s_per_thread", "toggles") if k in d}
    if a.note:
        rec["note"] = a.note
    print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()
