#!/usr/bin/env python3
"""Rate probe (dct3d_rate_frames_dev): the sizes of K candidate tables from one call against what the
codec offered before it, on device-resident 1920 x 1080 stacks (bench.py, the flagship measurement, is not
involved).

  (a)  one rate call with the K tables quant_table(q), q in --qualities
  (a') the same without the q = 1 table: what that table adds through its exact folds
  (b)  per table: set_quant, then encode_eg_frames_dev into a scratch stream, reading total_bits -- one context,
       so every table pays the plan rebuild and the table upload
  (c)  as (b) on K contexts prepared beforehand, one per table: the kernels alone.  The yardstick: (a) must be
       below it in every round of every configuration (the tool exits non-zero otherwise)

Configurations: grey (--grey-stacks) and packed RGB24 (--rgb-stacks) at each of --depths.  Before timing, (a)'s
bits summed over the stacks are checked against (c)'s totals, table by table and channel by channel.  Everything
runs on one stream shared by torch and the contexts, timed with device events; each variant is warmed up, then
`--rounds` rounds alternate the variants, `--iters` timed calls each, the round's figure being the median.  Prints
one JSON document; --out also writes it to a file."""
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
    ap.add_argument("--grey-stacks", type=int, default=126)
    ap.add_argument("--rgb-stacks", type=int, default=42)
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
        raise SystemExit("bench_rate.py needs a HIP device")
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

    res = {"tool": "bench_rate", "size": a.size, "iters": a.iters, "rounds": a.rounds, "qualities": qualities,
           "configs": []}
    ok = True
    with torch.cuda.stream(stream):
        for D in (int(d) for d in a.depths.split(",")):
            for C in (1, 3):
                n = a.grey_stacks if C == 1 else a.rgb_stacks
                tables = [pkg.quant_table(q, D) for q in qualities]
                no_q1 = [t for q, t in zip(qualities, tables) if q != 1]
                ctx = pkg.Context(0, 8, 8, D)
                ctx.set_stream(stream.cuda_stream)
                fr = content(ctx, D, C, n)
                cap = (fr.numel() // C * 3 + 64) // 4 * 4  # bytes per channel's scratch stream (24 bits a value)
                streams = [torch.zeros(cap // 4, dtype=torch.int32, device="cuda") for _ in range(C)]
                per_table = []
                for t in tables:
                    c = pkg.Context(0, 8, 8, D)
                    c.set_stream(stream.cuda_stream)
                    c.set_quant(t)
                    per_table.append(c)

                def va():
                    return ctx.rate_frames_dev(fr, W, H, C, n, tables)

                def va_no_q1():
                    return ctx.rate_frames_dev(fr, W, H, C, n, no_q1)

                def vb():
                    out = []
                    for t in tables:
                        ctx.set_quant(t)
                        out.append(ctx.encode_eg_frames_dev(fr, W, H, C, n, streams, [cap] * C))
                    return out

                def vc():
                    return [c.encode_eg_frames_dev(fr, W, H, C, n, streams, [cap] * C) for c in per_table]

                bits = va()
                st = ctx.stats()
                totals = vc()
                same = all(int(bits[t].sum(axis=0)[ch]) == totals[t][ch] for t in range(len(tables)) for ch in range(C))
                ctx.set_quant(None)
                variants = {"a_rate": va, "c_contexts": vc, "b_set_quant": vb}
                if len(no_q1) != len(tables) and no_q1:
                    variants["a_rate_without_q1"] = va_no_q1
                rounds = run_rounds(variants)
                ctx.set_quant(None)
                med = {k: statistics.median(v) for k, v in rounds.items()}
                below = all(x < y for x, y in zip(rounds["a_rate"], rounds["c_contexts"]))
                ok = ok and same and below
                cfg = {"depth": D, "channels": C, "stacks": n, "tables": len(tables),
                       "bits_equal_encoder_totals": bool(same),
                       "bits_per_pixel": {str(q): round(float(bits[t].sum()) / (fr.numel()), 4) for t, q in enumerate(qualities)},
                       "rate_stats": {"n_units": st["n_units"], "n_flagged": st["n_flagged"]},
                       "ms_per_round": rounds, "ms_median": med, "a_below_c_every_round": bool(below),
                       "a_over_c": round(med["a_rate"] / med["c_contexts"], 4),
                       "a_over_b": round(med["a_rate"] / med["b_set_quant"], 4),
                       "c_spread": round((max(rounds["c_contexts"]) - min(rounds["c_contexts"])) / med["c_contexts"], 4)}
                if "a_rate_without_q1" in med:
                    cfg["q1_adds_ms"] = round(med["a_rate"] - med["a_rate_without_q1"], 4)
                res["configs"].append(cfg)
                for c in per_table:
                    c.close()
                ctx.close()
                del fr, streams
                torch.cuda.empty_cache()

    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    if not ok:
        raise SystemExit("the rate call is not below the prepared contexts in every round, or its bits differ")


if __name__ == "__main__":
    main()
