"""Same-box measurements of the delivery to any device layout, on one GPU.  Three parts (--part):

  old       no regression on the contiguous path: the legs b (uint8, whole rows) and c (float16, scale 1/255, a 224-column
            window) of tools/decode_to_device_ab.py, through the calls WITHOUT a step (decode_batch_indexed_into,
            layout="rows"), on the parent commit's library (--parent-lib, through NBLIC_AMD_LIB) and on this tree's, in the
            three settings of profiles/r22_decode_to_device_ab.json (large: 16 frames of 4096 x 4096 at R = 64; small: 64 of
            1024 x 1024 at R = 32; rows: rows [300, 500) of those 64).  A library is chosen when the package is imported, so
            every (library, repetition) is a process of its own, the two alternating; a child makes its inputs, and per leg
            a fresh context, one warm-up and one timed run.
  layouts   P planes as P / 3 RGB frames (big: 48 planes of 4096 x 4096 at R = 64; small: 192 of 512 x 512 at R = 32) into a
            uint8 [N, H, W, 3] tensor and into a channels-last float16 [N, 3, H, W] tensor with a scale and bias per
            channel: straight there (nhwc_direct, cl16_direct: layout="any") against the planar call into a uint8
            [N, 3, H, W] scratch followed by the torch permute / normalisation into the same tensor (nhwc_torch,
            cl16_torch).  Wall time; what torch holds for the leg beyond the destination (the scratch) and its peak of
            temporaries; and Context.indexed_decode_split of every run, whose copy_out is the delivery launch (host ms around
            the launch and the wait for it): planar against interleaved on the same planes.
  recon     encode_batch_from at -n2 -e1 on 192 uint8 frames of 512 x 512 that lie on the device, with the reconstructions
            to a device tensor (recon_out) against the host recons.

The tensors are compared with the numpy expression on the inputs, bit for bit: in every run of old and recon, in the
warm-up and the last repetition of every leg of layouts.
Medians of --repeat runs with min-to-max spreads.  Each part and setting is one driver process; run each under its own time
limit and chain them, so that a fault ends the sequence:

    timeout -k 10 900 python tools/decode_layouts_ab.py --part old --setting large --parent-lib PARENT/libnblic_amd.so --out profiles/r24_decode_layouts_ab.json && \\
    timeout -k 10 600 python tools/decode_layouts_ab.py --part old --setting small --parent-lib PARENT/libnblic_amd.so --out profiles/r24_decode_layouts_ab.json && \\
    timeout -k 10 600 python tools/decode_layouts_ab.py --part old --setting rows --parent-lib PARENT/libnblic_amd.so --out profiles/r24_decode_layouts_ab.json && \\
    timeout -k 10 900 python tools/decode_layouts_ab.py --part layouts --setting big --out profiles/r24_decode_layouts_ab.json && \\
    timeout -k 10 600 python tools/decode_layouts_ab.py --part layouts --setting small --out profiles/r24_decode_layouts_ab.json && \\
    timeout -k 10 600 python tools/decode_layouts_ab.py --part recon --out profiles/r24_decode_layouts_ab.json

A result is merged into --out under "<part>_<setting>".
"""
import argparse, importlib, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="")
ap.add_argument("--part", choices=("old", "layouts", "recon"), default="layouts")
ap.add_argument("--setting", default="")
ap.add_argument("--repeat", type=int, default=3)
ap.add_argument("--parent-lib", default="")
ap.add_argument("--child", action="store_true")
ap.add_argument("--child-timeout", type=int, default=280)
args = ap.parse_args()

OLD = {"large": (16, 4096, 4096, 64, None), "small": (64, 1024, 1024, 32, None), "rows": (64, 1024, 1024, 32, (300, 500)), "quick": (6, 256, 256, 16, (80, 130))}
LAYOUTS = {"big": (48, 4096, 64), "small": (192, 512, 32), "quick": (6, 256, 16)}
NORMS = ((1.0 / 255.0 / 0.229, -0.485 / 0.229), (1.0 / 255.0 / 0.224, -0.456 / 0.224), (1.0 / 255.0 / 0.225, -0.406 / 0.225))     # (px / 255 - mean) / std
setting = args.setting or {"old": "large", "layouts": "big", "recon": "small"}[args.part]


def context(pkg):
    return pkg.Context(device=0, n_slots=48, n_coders=16, n_groups=6)


def median_of(runs, leg, key="wall_s"):
    t = [r[key] for r in runs if r["leg"] == leg]
    return {"runs": t, "median": round(statistics.median(t), 4), "min": min(t), "max": max(t), "spread": round(max(t) - min(t), 4)}


def merge(doc):
    if not args.out:
        return
    merged = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            merged = json.load(f)
    merged[f"{args.part}_{setting}"] = doc
    with open(args.out, "w") as f:
        json.dump(merged, f, indent=1)
        f.write("\n")


# ---- part old: one child per (library, repetition) --------------------------------------------------------------------------
def old_child():
    import numpy as np
    import torch
    torch.cuda.init()                                   # (torch first: the library binds to the HIP runtime that is already loaded)
    pkg = importlib.import_module("nblic-image-compression_amd")
    N, H, W, R, ROWS = OLD[setting]
    cols = ((W - 224) // 2 + 1, (W - 224) // 2 + 225)
    r0, r1 = ROWS if ROWS else (0, H)
    imgs = [pkg.syn1(H, W, 1 + k) for k in range(N)]
    ctx = context(pkg)
    pairs = ctx.encode_batch_indexed(imgs, R)
    ctx.close()
    want_u8 = np.stack([i[r0:r1] for i in imgs])
    want_f16 = (want_u8[:, :, cols[0]:cols[1]].astype(np.float32) * np.float32(1.0 / 255.0)).astype(np.float16)
    out_u8 = torch.empty((N, r1 - r0, W), dtype=torch.uint8, device="cuda")
    out_f16 = torch.empty((N, r1 - r0, 224), dtype=torch.float16, device="cuda")
    legs = {"b": lambda c: c.decode_batch_indexed_into(pairs, out_u8, rows=ROWS), "c": lambda c: c.decode_batch_indexed_into(pairs, out_f16, rows=ROWS, cols=cols, scale=1.0 / 255.0)}
    for leg, call in legs.items():
        ctx = context(pkg)
        try:
            assert call(ctx) == [0] * N                 # warm-up
            out_u8.zero_(); out_f16.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            status = call(ctx)
            wall = time.perf_counter() - t0
            split = ctx.indexed_decode_split()
        finally:
            ctx.close()
        got, want = (out_u8, want_u8) if leg == "b" else (out_f16, want_f16)
        assert status == [0] * N and (got.cpu().numpy().view(np.uint8) == want.view(np.uint8)).all(), leg
        print("RESULT " + json.dumps({"leg": leg, "wall_s": round(wall, 4), "split_ms": {k: round(v, 2) for k, v in split.items()}}), flush=True)


def old_driver():
    assert args.parent_lib, "--part old needs --parent-lib"
    runs = []
    for _ in range(args.repeat):
        for lib in ("parent", "tree"):
            env = dict(os.environ)
            env.pop("NBLIC_AMD_LIB", None)
            if lib == "parent":
                env["NBLIC_AMD_LIB"] = os.path.abspath(args.parent_lib)
            cmd = ["timeout", "-k", "10", str(args.child_timeout), sys.executable, os.path.abspath(__file__), "--part", "old", "--setting", setting, "--child"]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True)
            lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
            if r.returncode != 0 or len(lines) != 2:    # a fault, a time limit, a failed check: nothing more is started
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                raise SystemExit(f"the {lib} child ended with status {r.returncode}: the A/B stops here")
            for l in lines:
                rec = json.loads(l[len("RESULT "):])
                rec["leg"] = f"{lib}_{rec['leg']}"
                print(json.dumps(rec), flush=True)
                runs.append(rec)
    summary = {leg: median_of(runs, leg) for leg in ("parent_b", "tree_b", "parent_c", "tree_c")}
    verdict = {}
    for leg in ("b", "c"):
        slower = round(summary[f"tree_{leg}"]["median"] - summary[f"parent_{leg}"]["median"], 4)
        verdict[leg] = {"tree_slower_than_parent_by_s": slower, "parent_spread_s": summary[f"parent_{leg}"]["spread"],
                        "within_parent_spread": bool(slower <= summary[f"parent_{leg}"]["spread"])}
    N, H, W, R, ROWS = OLD[setting]
    doc = {"what": "decode_batch_indexed_into (layout rows) as tools/decode_to_device_ab.py's legs b and c, on the parent commit's library and on this tree's; a process "
                   "per (library, repetition), alternating; per leg a fresh context, one warm-up and one timed run; every tensor compared bit for bit",
           "frames": N, "h": H, "w": W, "every_rows": R, "rows": ROWS, "repeat": args.repeat, "runs": runs, "summary_wall_s": summary, "no_regression": verdict}
    print(json.dumps(verdict), flush=True)
    merge(doc)


# ---- part layouts: one process, the legs alternating -------------------------------------------------------------------------
def layouts():
    import numpy as np
    import torch
    torch.cuda.init()
    pkg = importlib.import_module("nblic-image-compression_amd")
    P, S, R = LAYOUTS[setting]
    N = P // 3
    base = [pkg.syn1(S, S, 1 + k) for k in range(min(P, 6))]
    imgs = [base[k % len(base)] for k in range(P)]
    ctx = context(pkg)
    pairs = ctx.encode_batch_indexed(imgs, R)
    ctx.close()
    assert all(ix is not None for _, ix in pairs)
    scales = [NORMS[c][0] for _ in range(N) for c in range(3)]
    biases = [NORMS[c][1] for _ in range(N) for c in range(3)]
    nhwc = torch.empty((N, S, S, 3), dtype=torch.uint8, device="cuda")
    cl16 = torch.empty((N, S, S, 3), dtype=torch.float16, device="cuda").permute(0, 3, 1, 2)      # [N, 3, H, W], channels last
    assert cl16.is_contiguous(memory_format=torch.channels_last)
    t_scale = torch.tensor([n[0] for n in NORMS], dtype=torch.float32, device="cuda").view(1, 3, 1, 1)
    t_bias = torch.tensor([n[1] for n in NORMS], dtype=torch.float32, device="cuda").view(1, 3, 1, 1)

    def nhwc_direct(c):
        assert c.decode_batch_indexed_into(pairs, nhwc.permute(0, 3, 1, 2), layout="any") == [0] * P
        return nhwc, 0

    def nhwc_torch(c):
        scratch = torch.empty((N, 3, S, S), dtype=torch.uint8, device="cuda")
        assert c.decode_batch_indexed_into(pairs, scratch.view(P, S, S)) == [0] * P
        nhwc.copy_(scratch.permute(0, 2, 3, 1))
        torch.cuda.synchronize()
        return nhwc, scratch.numel()

    def cl16_direct(c):
        assert c.decode_batch_indexed_into(pairs, cl16, layout="any", scale=scales, bias=biases) == [0] * P
        return cl16, 0

    def cl16_torch(c):
        scratch = torch.empty((N, 3, S, S), dtype=torch.uint8, device="cuda")
        assert c.decode_batch_indexed_into(pairs, scratch.view(P, S, S)) == [0] * P
        for ch in range(3):                             # (a channel at a time: the float32 temporaries are a third of the batch)
            cl16[:, ch].copy_(scratch[:, ch].float().mul_(t_scale[0, ch]).add_(t_bias[0, ch]))
        torch.cuda.synchronize()
        return cl16, scratch.numel()

    legs = {"nhwc_torch": nhwc_torch, "nhwc_direct": nhwc_direct, "cl16_torch": cl16_torch, "cl16_direct": cl16_direct}
    want_nhwc = np.stack(imgs).reshape(N, 3, S, S).transpose(0, 2, 3, 1)

    def check(name, res):
        got = res.cpu().numpy()
        if name.startswith("nhwc"):
            assert (got == want_nhwc).all(), name
            return
        for ch in range(3):                             # (a channel at a time: host memory)
            want = (want_nhwc[..., ch].astype(np.float32) * np.float32(NORMS[ch][0]) + np.float32(NORMS[ch][1])).astype(np.float16)
            assert (got[:, ch].view(np.uint16) == want.view(np.uint16)).all(), (name, ch)

    def run(name, checked=True):
        ctx = context(pkg)
        try:
            nhwc.zero_(); cl16.zero_()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            held = torch.cuda.memory_allocated()
            t0 = time.perf_counter()
            res, scratch_bytes = legs[name](ctx)
            wall = time.perf_counter() - t0
            peak = torch.cuda.max_memory_allocated() - held
            split = ctx.indexed_decode_split()
            stats = ctx.deliver_stats()
        finally:
            ctx.close()
        if checked:
            check(name, res)
        rec = {"leg": name, "checked": checked, "wall_s": round(wall, 4), "torch_peak_extra_bytes": int(peak), "scratch_bytes": int(scratch_bytes), "deliver_tasks": list(stats),
               "split_ms": {k: round(v, 3) for k, v in split.items()}, "delivery_ms": round(split["copy_out"], 3)}
        print(json.dumps(rec), flush=True)
        return rec

    warm = [run(name) for name in legs]
    runs = [run(name, checked=(k == args.repeat - 1)) for k in range(args.repeat) for name in legs]       # (the host's comparison of a large batch takes longer than its run)
    summary = {name: {"wall_s": median_of(runs, name), "delivery_ms": median_of(runs, name, "delivery_ms"),
                      "torch_peak_extra_bytes": max(r["torch_peak_extra_bytes"] for r in runs if r["leg"] == name),
                      "rounds_ms_median": round(statistics.median(r["split_ms"]["rounds"] for r in runs if r["leg"] == name), 2)} for name in legs}
    compare = {}
    for kind in ("nhwc", "cl16"):
        old, new = summary[kind + "_torch"], summary[kind + "_direct"]
        gain = round(old["wall_s"]["median"] - new["wall_s"]["median"], 4)
        compare[kind] = {"torch_over_direct_ratio_of_medians": round(old["wall_s"]["median"] / new["wall_s"]["median"], 3), "gain_s": gain,
                         "spread_of_torch_leg_s": old["wall_s"]["spread"], "gain_exceeds_spread": bool(gain > old["wall_s"]["spread"]),
                         "extra_device_bytes_torch": old["torch_peak_extra_bytes"], "extra_device_bytes_direct": new["torch_peak_extra_bytes"],
                         "delivery_ms_planar": old["delivery_ms"]["median"], "delivery_ms_interleaved": new["delivery_ms"]["median"],
                         "interleaved_over_planar_delivery": round(new["delivery_ms"]["median"] / max(old["delivery_ms"]["median"], 1e-9), 2),
                         "interleaved_delivery_share_of_the_call": round(new["delivery_ms"]["median"] / 1e3 / new["wall_s"]["median"], 5)}
    doc = {"what": "P planes as P / 3 RGB frames through decode_batch_indexed_into: straight into uint8 NHWC / channels-last float16 with a scale and bias per channel "
                   "(x_direct, layout any) against the planar call into a uint8 scratch followed by the torch permute / normalisation into the same tensor (x_torch); one "
                   "process, a fresh context of 6 groups x 8 slots and 16 coder threads per leg and run, destinations allocated once, one warm-up per leg, then the runs "
                   "alternating; the tensors of the warm-up and of the last repetition compared with the numpy expression bit for bit.  delivery_ms is indexed_decode_split's copy_out: host ms around the "
                   "k_deliver launch and the wait for it",
           "planes": P, "frames": N, "h": S, "w": S, "every_rows": R, "norms": NORMS, "repeat": args.repeat, "warm_up": warm, "runs": runs, "summary": summary, "direct_against_torch": compare}
    print(json.dumps(compare), flush=True)
    merge(doc)


# ---- part recon: reconstructions of a near-lossless encode, to the device against to the host --------------------------------
def recon():
    import numpy as np
    import torch
    torch.cuda.init()
    pkg = importlib.import_module("nblic-image-compression_amd")
    P, S = (192, 512) if setting != "quick" else (6, 256)
    base = [pkg.syn1(S, S, 1 + k) for k in range(min(P, 6))]
    src = torch.from_numpy(np.stack([base[k % len(base)] for k in range(P)])).cuda()
    out = torch.empty((P, S, S), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def host(c):
        info = {}
        streams = c.encode_batch_from(src, near=2, effort=1, info=info)
        return streams, np.stack(info["recons"])

    def device(c):
        streams = c.encode_batch_from(src, near=2, effort=1, recon_out=out)
        return streams, None

    legs = {"recon_host": host, "recon_device": device}
    first = {}

    def run(name):
        ctx = context(pkg)
        try:
            legs[name](ctx)                             # warm-up
            out.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            streams, rec = legs[name](ctx)
            wall = time.perf_counter() - t0
        finally:
            ctx.close()
        rec = out.cpu().numpy() if rec is None else rec
        first.setdefault("streams", streams); first.setdefault("recon", rec)
        assert streams == first["streams"] and (rec == first["recon"]).all(), name
        r = {"leg": name, "wall_s": round(wall, 4), "mpixel_per_s": round(P * S * S / wall / 1e6, 1)}
        print(json.dumps(r), flush=True)
        return r

    runs = [run(name) for _ in range(args.repeat) for name in legs]
    summary = {name: median_of(runs, name) for name in legs}
    gain = round(summary["recon_host"]["median"] - summary["recon_device"]["median"], 4)
    doc = {"what": "encode_batch_from at -n2 -e1 on P uint8 frames on the device: the reconstructions to host buffers (recon_host) against recon_out, a uint8 device tensor "
                   "(recon_device); one process, a fresh context per leg and run with one warm-up call in it, alternating; streams and reconstructions of every run are the same bytes",
           "frames": P, "h": S, "w": S, "repeat": args.repeat, "runs": runs, "summary_wall_s": summary,
           "device_against_host": {"ratio_of_medians": round(summary["recon_host"]["median"] / summary["recon_device"]["median"], 3), "gain_s": gain,
                                   "spread_of_host_leg_s": summary["recon_host"]["spread"], "gain_exceeds_spread": bool(gain > summary["recon_host"]["spread"]),
                                   "host_bytes_for_reconstructions": P * S * S}}
    print(json.dumps(doc["device_against_host"]), flush=True)
    merge(doc)


if args.part == "old":
    old_child() if args.child else old_driver()
elif args.part == "layouts":
    layouts()
else:
    recon()
