#!/usr/bin/env python3
"""Distortion probe (dct3d_distortion_frames_dev): the exact squared error of encode + decode under K
candidate tables from one call against what the library offered before it, on device-resident 1920 x 1080 stacks
(bench.py, the flagship measurement, is not involved).

  (a)  one probe call with the K tables quant_table(q), q in --qualities
  (a1) the same with the first table alone: (a - a1) / (K - 1) is what one more table costs
  (c)  per table, on K contexts prepared beforehand (no plan rebuild in the timing): encode_frames_dev to int32,
       decode_frames_dev to a raster, a torch squared-difference reduction per (stack, channel).  The yardstick:
       (a) must be below it in every round of every configuration (the tool exits non-zero otherwise)

Configurations: grey (--grey-stacks) and packed RGB24 (--rgb-stacks) at each of --depths.  Before timing, (a)'s
sums are checked against (c)'s, table by table, stack by stack and channel by channel.  Everything runs on one
stream shared by torch and the contexts, timed with device events; each variant is warmed up, then `--rounds`
rounds alternate the variants, `--iters` timed calls each, the round's figure being the median.  Prints one JSON
document; --out also writes it to a file."""
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
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--grey-stacks", type=int, default=32)
    ap.add_argument("--rgb-stacks", type=int, default=12)
    ap.add_argument("--depths", default="8,4")
    ap.add_argument("--qualities", default="1,2,3,5,8,12,20,32")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    W, H = (int(v) for v in a.size.split("x"))
    qualities = [int(q) for q in a.qualities.split(",")]

    import torch
    pkg = importlib.import_module("3ddctvideoencoding_amd")
    if not torch.cuda.is_available():
        raise SystemExit("bench_distortion.py needs a HIP device")
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

    def content(ctx, D, C, n):
        F = n * D
        if C == 1:
            t = torch.empty((F, H, W), dtype=torch.uint8, device="cuda")
            ctx.fill_synthetic_dev(t, W, H, F, kind="ramp")
            return t
        planes = torch.empty((3, F, H, W), dtype=torch.uint8, device="cuda")
        ctx.fill_synthetic_dev(planes[0], W, H, F, kind="ramp")
        ctx.fill_synthetic_dev(planes[1], W, H, F, seed=0x77A1, frame0=3, kind="uniform")
        ctx.fill_synthetic_dev(planes[2], W, H, F, seed=0x51DE5, frame0=11, kind="ramp")
        return planes.permute(1, 2, 3, 0).contiguous()

    res = {"tool": "bench_distortion", "size": a.size, "iters": a.iters, "rounds": a.rounds, "qualities": qualities,
           "configs": []}
    ok = True
    wp, hp = pkg.padded_size(W, H)
    with torch.cuda.stream(stream):
        for D in (int(d) for d in a.depths.split(",")):
            for C in (1, 3):
                n = a.grey_stacks if C == 1 else a.rgb_stacks
                tables = [pkg.quant_table(q, D) for q in qualities]
                ctx = pkg.Context(0, 8, 8, D)
                ctx.set_stream(stream.cuda_stream)
                fr = content(ctx, D, C, n)
                d_q = torch.empty(C * n * D * hp * wp, dtype=torch.int32, device="cuda")
                d_out = torch.empty_like(fr)
                per_table = []
                for t in tables:
                    c = pkg.Context(0, 8, 8, D)
                    c.set_stream(stream.cuda_stream)
                    c.set_quant(t)
                    per_table.append(c)

                def va():
                    return ctx.distortion_frames_dev(fr, W, H, C, n, tables)

                def va1():
                    return ctx.distortion_frames_dev(fr, W, H, C, n, tables[:1])

                def vc():
                    out = []
                    for c in per_table:
                        c.encode_frames_dev(fr, W, H, C, n, d_q)
                        c.decode_frames_dev(d_q, W, H, C, n, d_out)
                        d = fr.to(torch.int32) - d_out.to(torch.int32)
                        out.append((d * d).view(n, D * H * W, C).sum(dim=1, dtype=torch.int64))  # [stack, channel]
                    return torch.stack(out).cpu().numpy()  # one read-back, as the probe's

                sse = va()
                st = ctx.stats()
                want = vc()
                same = bool((sse.astype("int64") == want).all())
                variants = {"a_probe": va, "c_contexts": vc}
                if len(tables) > 1:
                    variants["a1_one_table"] = va1
                rounds = run_rounds(variants)
                med = {k: statistics.median(v) for k, v in rounds.items()}
                below = all(x < y for x, y in zip(rounds["a_probe"], rounds["c_contexts"]))
                ok = ok and same and below
                cfg = {"depth": D, "channels": C, "stacks": n, "tables": len(tables),
                       "sse_equal_yardstick": same,
                       "psnr_db": {str(q): round(pkg.psnr_db(int(sse[t].sum()), fr.numel()), 3) for t, q in enumerate(qualities)},
                       "probe_stats": {"n_units": st["n_units"], "n_flagged": st["n_flagged"]},
                       "ms_per_round": rounds, "ms_median": med, "a_below_c_every_round": bool(below),
                       "a_over_c": round(med["a_probe"] / med["c_contexts"], 4),
                       "a_spread": round((max(rounds["a_probe"]) - min(rounds["a_probe"])) / med["a_probe"], 4),
                       "c_spread": round((max(rounds["c_contexts"]) - min(rounds["c_contexts"])) / med["c_contexts"], 4)}
                if "a1_one_table" in med:
                    cfg["ms_per_more_table"] = round((med["a_probe"] - med["a1_one_table"]) / (len(tables) - 1), 4)
                res["configs"].append(cfg)
                for c in per_table:
                    c.close()
                ctx.close()
                del fr, d_q, d_out
                torch.cuda.empty_cache()

    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    if not ok:
        raise SystemExit("the probe is not below the prepared contexts in every round, or its sums differ")


if __name__ == "__main__":
    main()
