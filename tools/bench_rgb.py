#!/usr/bin/env python3
"""Packed RGB24 encode / decode against what the project could do without them, on device-resident 1080p x 8
stacks (bench.py, the flagship measurement, is not involved).

  (a) fused RGB encode        encode_stacks_rgb_dev
  (b) split-path encode       torch de-interleave to planar (permute(...).contiguous()) + encode_stacks_dev on 3n
                              planar stacks: the baseline
  (c) grey encode             encode_stacks_dev on the same number of bytes: the ceiling
  (d) fused RGB decode        decode_stacks_rgb_dev
  (e) split-path decode       decode_stacks_dev on 3n planar stacks + torch re-interleave
  (f) grey decode             the ceiling

Everything runs on one stream shared by torch and the context, timed with device events; each shape is warmed
up, then `--rounds` rounds alternate the variants (A/B x rounds), `--iters` timed calls each, the round's
figure being the median.  Before timing, (a) is compared with (b) and (d) with (e), bit for bit, at the timed
size.  Prints one JSON document; --out also writes it to a file.

  --only a|b|c|d|e|f   run just that variant, untimed loops of --iters calls (for a profiler run of its own)
"""
import argparse
import importlib
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stacks", type=int, default=42, help="RGB stacks (grey: 3x as many); 42 ~ the c2 step")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--depth", type=int, default=8, choices=(8, 4))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    pkg = importlib.import_module("3ddctvideoencoding_amd")
    if not torch.cuda.is_available():
        raise SystemExit("bench_rgb.py needs a HIP device")
    W, H, D, n = a.width, a.height, a.depth, a.stacks
    F = n * D
    stream = torch.cuda.Stream()
    ctx = pkg.Context(0, 8, 8, D)
    ctx.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        # content: R ramp, G uniform noise, B another ramp (planar first, then packed)
        planes = torch.empty((3, F, H, W), dtype=torch.uint8, device="cuda")
        ctx.fill_synthetic_dev(planes[0], W, H, F, kind="ramp")
        ctx.fill_synthetic_dev(planes[1], W, H, F, seed=0x77A1, frame0=3, kind="uniform")
        ctx.fill_synthetic_dev(planes[2], W, H, F, seed=0x51DE5, frame0=11, kind="ramp")
        d_rgb = planes.permute(1, 2, 3, 0).contiguous()                       # [F, H, W, 3]
        d_grey = d_rgb.view(3 * F, H, W)                                      # the same bytes read as grey frames
        del planes
        n_cubes = ctx.n_cubes(W, H, n)
        d_q = torch.empty((3 * n_cubes, D, 8, 8), dtype=torch.int32, device="cuda")
        d_q2 = torch.empty_like(d_q)
        d_out = torch.empty_like(d_rgb)
        d_planar = torch.empty((3 * F, H, W), dtype=torch.uint8, device="cuda")

        def enc_fused():
            ctx.encode_stacks_rgb_dev(d_rgb, W, H, n, d_q)

        def enc_split():
            pl = d_rgb.view(n, D, H, W, 3).permute(0, 4, 1, 2, 3).contiguous()
            ctx.encode_stacks_dev(pl, W, H, 3 * n, d_q2)

        def enc_grey():
            ctx.encode_stacks_dev(d_grey, W, H, 3 * n, d_q2)

        def dec_fused():
            ctx.decode_stacks_rgb_dev(d_q, W, H, n, d_out)

        def dec_split():
            ctx.decode_stacks_dev(d_q, W, H, 3 * n, d_planar)
            d_out.view(n, D, H, W, 3).copy_(d_planar.view(n, 3, D, H, W).permute(0, 2, 3, 4, 1))

        def dec_grey():
            ctx.decode_stacks_dev(d_q, W, H, 3 * n, d_planar)

        variants = {"a": enc_fused, "b": enc_split, "c": enc_grey, "d": dec_fused, "e": dec_split, "f": dec_grey}
        names = {"a": "enc_fused_rgb", "b": "enc_split_baseline", "c": "enc_grey_ceiling",
                 "d": "dec_fused_rgb", "e": "dec_split_baseline", "f": "dec_grey_ceiling"}

        if a.only:
            enc_fused()  # d_q for the decodes
            for _ in range(a.iters):
                variants[a.only]()
            stream.synchronize()
            print(json.dumps({"only": names[a.only], "iters": a.iters}))
            return

        # results must not differ: fused == split path, at the timed size
        enc_fused()
        enc_split()
        enc_equal = bool(torch.equal(d_q, d_q2))
        dec_fused()
        ref = d_out.clone()
        d_out.zero_()
        dec_split()
        dec_equal = bool(torch.equal(ref, d_out))
        del ref

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

        for k in variants:
            for _ in range(a.warmup):
                variants[k]()
        stream.synchronize()
        rounds = {names[k]: [] for k in variants}
        for _ in range(a.rounds):
            for k in variants:  # alternate the variants within a round
                rounds[names[k]].append(round(timed(variants[k]), 4))

    samples = 3 * n_cubes * ctx.cube_size
    med = {k: statistics.median(v) for k, v in rounds.items()}
    res = {
        "tool": "bench_rgb", "width": W, "height": H, "depth": D, "rgb_stacks": n, "grey_stacks": 3 * n,
        "samples": samples, "iters": a.iters, "rounds": a.rounds, "ms_per_round": rounds, "ms_median": med,
        "algorithmic_bytes_per_sample": {"fused": 5, "split": 7, "grey": 5},
        "fused_GBps": {k: round(5 * samples / (med[k] * 1e6), 1) for k in ("enc_fused_rgb", "dec_fused_rgb")},
        "enc_fused_over_split": round(med["enc_fused_rgb"] / med["enc_split_baseline"], 4),
        "enc_fused_over_grey": round(med["enc_fused_rgb"] / med["enc_grey_ceiling"], 4),
        "dec_fused_over_split": round(med["dec_fused_rgb"] / med["dec_split_baseline"], 4),
        "dec_fused_over_grey": round(med["dec_fused_rgb"] / med["dec_grey_ceiling"], 4),
        "enc_fused_faster_every_round": all(x < y for x, y in zip(rounds["enc_fused_rgb"], rounds["enc_split_baseline"])),
        "dec_fused_faster_every_round": all(x < y for x, y in zip(rounds["dec_fused_rgb"], rounds["dec_split_baseline"])),
        "enc_fused_equals_split": enc_equal, "dec_fused_equals_split": dec_equal,
    }
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    ctx.close()
    if not (enc_equal and dec_equal):
        raise SystemExit("fused and split-path results differ")


if __name__ == "__main__":
    main()
