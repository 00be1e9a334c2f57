#!/usr/bin/env python3
"""RGB-domain distortion probe (dct3d_distortion_rgb_frames_dev): the exact squared error in the RGB
pixels under K (Y, Cb, Cr) table triples from one call against what the library offered before it, on
device-resident 1920 x 1080 packed RGB24 stacks (bench.py, the flagship measurement, is not involved).

  (a)  one probe call with the K candidates (quant_table(q_i), quant_table(q_j), quant_table(q_j)), q in --qualities,
       j = min(i + chroma_rungs, K - 1), for each of --rungs
  (a1) the same with the first candidate alone
  (c)  the yardstick, the library at its best without the probe: per candidate encode_eg_frames_vqc_dev +
       decode_eg_frames_vqc_dev with a constant map, and a torch squared-difference reduction per stack
  (c0) (c) without the squared difference: the stream calls alone (what part of (c) is the library's)

Configurations: YCbCr 4:4:4 and 4:2:0 at each of --depths.  Before timing, (a)'s sums are checked against (c)'s,
candidate by candidate and stack by stack (the tool exits non-zero when they differ; whether (a) is below (c) is
recorded, not required).  Everything runs on one stream shared by torch and the contexts, timed with device events;
each variant is warmed up, then `--rounds` rounds alternate the variants, `--iters` timed calls each, the round's
figure being the median.  Prints one JSON document; --out also writes it to a file."""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--stacks", type=int, default=4)
    ap.add_argument("--depths", default="8,4")
    ap.add_argument("--qualities", default="1,2,3,5,8,12,20,32")
    ap.add_argument("--rungs", default="0,2")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    W, H = (int(v) for v in a.size.split("x"))
    qualities = [int(q) for q in a.qualities.split(",")]
    K = len(qualities)

    import torch
    pkg = importlib.import_module("3ddctvideoencoding_amd")
    if not torch.cuda.is_available():
        raise SystemExit("bench_distortion_rgb.py needs a HIP device")
    stream = torch.cuda.Stream()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms = []
        for _ in range(a.iters):
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return statistics.median(ms)

    def run_rounds(variants):
        for fn in variants.values():
            for _ in range(a.warmup):
                fn()
        stream.synchronize()
        rounds = {k: [] for k in variants}
        for _ in range(a.rounds):
            for k, fn in variants.items():  # alternate the variants within a round
                rounds[k].append(round(timed(fn), 4))
        return rounds

    def content(ctx, D, n):
        F = n * D
        planes = torch.empty((3, F, H, W), dtype=torch.uint8, device="cuda")
        ctx.fill_synthetic_dev(planes[0], W, H, F, kind="ramp")
        ctx.fill_synthetic_dev(planes[1], W, H, F, seed=0x77A1, frame0=3, kind="uniform")
        ctx.fill_synthetic_dev(planes[2], W, H, F, seed=0x51DE5, frame0=11, kind="ramp")
        return planes.permute(1, 2, 3, 0).contiguous()

    res = {"tool": "bench_distortion_rgb", "size": a.size, "stacks": a.stacks, "iters": a.iters, "rounds": a.rounds,
           "qualities": qualities, "configs": []}
    ok = True
    wp, hp = pkg.padded_size(W, H)
    n = a.stacks
    with torch.cuda.stream(stream):
        for D in (int(d) for d in a.depths.split(",")):
            for chroma in ("444", "420"):
                tables = [pkg.quant_table(q, D) for q in qualities]
                ctx = pkg.Context(0, 8, 8, D)
                ctx.set_stream(stream.cuda_stream)
                ctx.set_option(pkg.DCT3D_OPT_COLOUR, pkg.DCT3D_COLOUR_YCBCR)
                ctx.set_chroma(pkg.DCT3D_CHROMA_420 if chroma == "420" else pkg.DCT3D_CHROMA_444)
                fr = content(ctx, D, n)
                d_out = torch.empty_like(fr)
                cap = wp * hp * D * n * 4 + 64  # holds any content: 4 bytes per value of the padded plane
                d_streams = [torch.empty(cap, dtype=torch.uint8, device="cuda") for _ in range(3)]
                for rungs in (int(r) for r in a.rungs.split(",")):
                    cand = [(i, min(i + rungs, K - 1), min(i + rungs, K - 1)) for i in range(K)]

                    def va():
                        return ctx.distortion_rgb_frames_dev(fr, W, H, n, tables, cand)

                    def va1():
                        return ctx.distortion_rgb_frames_dev(fr, W, H, n, tables, cand[:1])

                    def vc(diff=True):
                        out = []
                        for c in cand:
                            m = np.tile(np.array(c, np.uint8), (n, 1))
                            tb = ctx.encode_eg_frames_vqc_dev(fr, W, H, 3, n, tables, m, d_streams, [cap] * 3)
                            ctx.decode_eg_frames_vqc_dev(d_streams, [(t + 7) // 8 for t in tb], [0] * 3, W, H, n, tables, m, d_out)
                            if diff:
                                d = fr.to(torch.int32) - d_out.to(torch.int32)
                                out.append((d * d).view(n, -1).sum(dim=1, dtype=torch.int64))
                        return torch.stack(out).cpu().numpy() if diff else None  # one read-back, as the probe's

                    def vc0():
                        return vc(False)

                    sse = va()
                    st = ctx.stats()
                    same = bool((sse.astype("int64") == vc()).all())
                    rounds = run_rounds({"a_probe": va, "c_stream_calls": vc, "a1_one_candidate": va1, "c0_stream_calls_alone": vc0})
                    med = {k: statistics.median(v) for k, v in rounds.items()}
                    below = all(x < y for x, y in zip(rounds["a_probe"], rounds["c_stream_calls"]))
                    ok = ok and same
                    res["configs"].append({
                        "depth": D, "chroma": chroma, "chroma_rungs": rungs, "stacks": n, "candidates": K,
                        "sse_equal_yardstick": same,
                        "psnr_db": {str(q): round(pkg.psnr_db(int(sse[t].sum()), fr.numel()), 3) for t, q in enumerate(qualities)},
                        "probe_stats": {"n_units": st["n_units"], "n_flagged": st["n_flagged"]},
                        "ms_per_round": rounds, "ms_median": med, "a_below_c_every_round": bool(below),
                        "a_over_c": round(med["a_probe"] / med["c_stream_calls"], 4),
                        "a_over_c0": round(med["a_probe"] / med["c0_stream_calls_alone"], 4),
                        "a_spread": round((max(rounds["a_probe"]) - min(rounds["a_probe"])) / med["a_probe"], 4),
                        "c_spread": round((max(rounds["c_stream_calls"]) - min(rounds["c_stream_calls"])) / med["c_stream_calls"], 4),
                        "ms_per_more_candidate": round((med["a_probe"] - med["a1_one_candidate"]) / (K - 1), 4) if K > 1 else None})
                ctx.close()
                del fr, d_out, d_streams
                torch.cuda.empty_cache()

    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    if not ok:
        raise SystemExit("the probe's sums differ from the stream calls'")


if __name__ == "__main__":
    main()
