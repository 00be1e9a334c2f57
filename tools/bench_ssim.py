#!/usr/bin/env python3
"""SSIM probe (dct3d_ssim_frames_dev): the exact windowed SSIM of encode + decode under K candidate tables
from one call against what the library offered before it, on device-resident 1920 x 1080 stacks (bench.py, the
flagship measurement, is not involved).  tools/bench_distortion.py's protocol.

  (a)  one SSIM probe call with the K tables quant_table(q), q in --qualities
  (a1) the same with the first table alone: (a - a1) / (K - 1) is what one more table costs
  (b)  distortion_frames_dev with (a)'s arguments: a / b is what the SSIM costs on top of the squared error
  (c)  per table, on K contexts prepared beforehand (no plan rebuild in the timing): encode_frames_dev to int32,
       decode_frames_dev to a raster, and the same windows in torch: 4 x 4 block moments by reshape sums (fp32, exact:
       16 x 255^2 < 2^24), the windows' sums, A, B, C, D in int64, the fp64 expression, floor, the sum per (stack,
       channel).  The yardstick: (a) must be below it in every round of every configuration (the tool exits non-zero
       otherwise)

Configurations: grey (--grey-stacks) and packed RGB24 (--rgb-stacks) at each of --depths.  Before timing, (a)'s sums
are checked against (c)'s, table by table, stack by stack and channel by channel.  Everything runs on one stream
shared by torch and the contexts, timed with device events; each variant is warmed up, then `--rounds` rounds
alternate the variants, `--iters` timed calls each, the round's figure being the median.  Prints one JSON document;
--out also writes it to a file."""
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
    import torch.nn.functional as F
    pkg = importlib.import_module("3ddctvideoencoding_amd")
    if not torch.cuda.is_available():
        raise SystemExit("bench_ssim.py needs a HIP device")
    stream = torch.cuda.Stream()
    nbx, nby = (W + 3) // 4, (H + 3) // 4
    nwx, nwy = pkg.ssim_windows(W, H)

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
        Fn = n * D
        if C == 1:
            t = torch.empty((Fn, H, W), dtype=torch.uint8, device="cuda")
            ctx.fill_synthetic_dev(t, W, H, Fn, kind="ramp")
            return t
        planes = torch.empty((3, Fn, H, W), dtype=torch.uint8, device="cuda")
        ctx.fill_synthetic_dev(planes[0], W, H, Fn, kind="ramp")
        ctx.fill_synthetic_dev(planes[1], W, H, Fn, seed=0x77A1, frame0=3, kind="uniform")
        ctx.fill_synthetic_dev(planes[2], W, H, Fn, seed=0x51DE5, frame0=11, kind="ramp")
        return planes.permute(1, 2, 3, 0).contiguous()

    def blocks(t):  # fp32 [P, H, W] -> the 4 x 4 blocks' sums, int64 [P, nby, nbx] (zero outside the frame)
        t = F.pad(t, (0, 4 * nbx - W, 0, 4 * nby - H))
        return t.view(-1, nby, 4, nbx, 4).sum(dim=(2, 4)).to(torch.int64)

    def windows(b):  # blocks -> windows: the 1, 2 or 4 blocks of each
        r = b[:, :nwy, :nwx].clone()
        if nbx > 1:
            r += b[:, :nwy, 1:nwx + 1]
        if nby > 1:
            r += b[:, 1:nwy + 1, :nwx]
        if nbx > 1 and nby > 1:
            r += b[:, 1:nwy + 1, 1:nwx + 1]
        return r

    def planes_of(t, C):  # u8 frames [F, H, W] or [F, H, W, 3] -> fp32 [F * C, H, W], plane (f, ch) at f * C + ch
        t = t.to(torch.float32)
        return t if C == 1 else t.permute(0, 3, 1, 2).reshape(-1, H, W)

    res = {"tool": "bench_ssim", "size": a.size, "iters": a.iters, "rounds": a.rounds, "qualities": qualities,
           "configs": []}
    ok = True
    wp, hp = pkg.padded_size(W, H)
    with torch.cuda.stream(stream):
        n_win = windows(blocks(torch.ones((1, H, W), dtype=torch.float32, device="cuda")))  # [1, nwy, nwx]
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
                    return ctx.ssim_frames_dev(fr, W, H, C, n, tables)

                def va1():
                    return ctx.ssim_frames_dev(fr, W, H, C, n, tables[:1])

                def vb():
                    return ctx.distortion_frames_dev(fr, W, H, C, n, tables)

                def vc():
                    out = []
                    for c in per_table:
                        c.encode_frames_dev(fr, W, H, C, n, d_q)
                        c.decode_frames_dev(d_q, W, H, C, n, d_out)
                        x, y = planes_of(fr, C), planes_of(d_out, C)
                        Sx, Sy = windows(blocks(x)), windows(blocks(y))
                        Sxx, Syy, Sxy = windows(blocks(x * x)), windows(blocks(y * y)), windows(blocks(x * y))
                        n2 = n_win * n_win
                        A = 20000 * Sx * Sy + 65025 * n2
                        B = 20000 * (n_win * Sxy - Sx * Sy) + 585225 * n2
                        Cc = 10000 * (Sx * Sx + Sy * Sy) + 65025 * n2
                        Dd = 10000 * (n_win * Sxx - Sx * Sx + n_win * Syy - Sy * Sy) + 585225 * n2
                        s = (A.double() * B.double()) / (Cc.double() * Dd.double())
                        v = torch.floor(s * 16777216.0).to(torch.int64)  # [F * C, nwy, nwx]
                        out.append(v.view(n, D, C, nwy * nwx).sum(dim=(1, 3)))  # [stack, channel]
                    return torch.stack(out).cpu().numpy()  # one read-back, as the probe's

                ssim = va()
                st = ctx.stats()
                want = vc()
                same = bool((ssim == want).all())
                variants = {"a_probe": va, "b_sse_probe": vb, "c_contexts": vc}
                if len(tables) > 1:
                    variants["a1_one_table"] = va1
                rounds = run_rounds(variants)
                med = {k: statistics.median(v) for k, v in rounds.items()}
                below = all(x < y for x, y in zip(rounds["a_probe"], rounds["c_contexts"]))
                ok = ok and same and below
                per_cfg = nwx * nwy * n * D * C
                cfg = {"depth": D, "channels": C, "stacks": n, "tables": len(tables),
                       "ssim_equal_yardstick": same,
                       "ssim_mean": {str(q): round(pkg.ssim_mean(int(ssim[t].sum()), per_cfg), 6) for t, q in enumerate(qualities)},
                       "probe_stats": {"n_units": st["n_units"], "n_flagged": st["n_flagged"]},
                       "ms_per_round": rounds, "ms_median": med, "a_below_c_every_round": bool(below),
                       "a_over_c": round(med["a_probe"] / med["c_contexts"], 4),
                       "a_over_b": round(med["a_probe"] / med["b_sse_probe"], 4),
                       "a_spread": round((max(rounds["a_probe"]) - min(rounds["a_probe"])) / med["a_probe"], 4),
                       "b_spread": round((max(rounds["b_sse_probe"]) - min(rounds["b_sse_probe"])) / med["b_sse_probe"], 4),
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
