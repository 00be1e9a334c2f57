#!/usr/bin/env python3
"""Per-stack quantiser tables (dct3d_*_eg_frames_vq_dev) against what the project offered before them, on
device-resident 1920 x 1080 stacks (bench.py, the flagship measurement, is not involved).  The palette is the
codec's 16-step ladder, the clip 16 stacks; encode and decode are timed separately:

  (a)  the vq call with a CONSTANT map (every stack the ladder's q = 5 entry)
  (b)  the QT = 1 kernels: a context under set_quant of that table, the base call on the same buffers.  The yardstick
       of (a): a / b is the cost of choosing the table per cube when nothing is chosen
  (c)  the vq call with a map CYCLING through the ladder
  (d)  the parent's best for that job: 16 contexts prepared beforehand (one per table), one single-stack base call
       per stack, the carry of each handed to the next (a one-byte read-back per stack: the chain needs it).  The
       yardstick of (c): (c) must be below (d) in every round (the tool exits non-zero otherwise)

Before timing, (a)'s streams and frames are compared with (b)'s and (c)'s with (d)'s, for equality.  Everything runs
on one stream shared by torch and the contexts, timed with device events; each variant is warmed up, then `--rounds`
rounds alternate the variants, `--iters` timed calls each, the round's figure being the median.  Prints one JSON
document; --out also writes it to a file."""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

LADDER = (1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 20, 24, 32, 40, 48, 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--stacks", type=int, default=16)
    ap.add_argument("--depths", default="8,4")
    ap.add_argument("--channels", default="1,3")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    W, H = (int(v) for v in a.size.split("x"))
    n = a.stacks

    import torch
    pkg = importlib.import_module("3ddctvideoencoding_amd")
    if not torch.cuda.is_available():
        raise SystemExit("bench_vq.py needs a HIP device")
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

    def content(ctx, D, C):
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

    res = {"tool": "bench_vq", "size": a.size, "stacks": n, "iters": a.iters, "rounds": a.rounds, "ladder": list(LADDER),
           "configs": []}
    ok = True
    with torch.cuda.stream(stream):
        for D in (int(d) for d in a.depths.split(",")):
            for C in (int(c) for c in a.channels.split(",")):
                pal = np.stack([pkg.quant_table(q, D) for q in LADDER]).astype(np.int32)
                const = np.full(n, LADDER.index(5), np.uint8)
                cyc = (np.arange(n) % len(LADDER)).astype(np.uint8)
                ctx = pkg.Context(0, 8, 8, D)
                ctx.set_stream(stream.cuda_stream)
                ctx_q = pkg.Context(0, 8, 8, D)
                ctx_q.set_stream(stream.cuda_stream)
                ctx_q.set_quant(pal[const[0]])
                per_table = []
                for t in pal:
                    c = pkg.Context(0, 8, 8, D)
                    c.set_stream(stream.cuda_stream)
                    c.set_quant(t)
                    per_table.append(c)
                fr = content(ctx, D, C)
                stack_elems = fr.numel() // n
                cap = (fr.numel() // C * 3 + 64) // 4 * 4          # bytes per channel's stream (24 bits a value)
                cap1 = (stack_elems // C * 3 + 64) // 4 * 4        # ... of one stack
                outs = {k: [torch.zeros(cap // 4, dtype=torch.int32, device="cuda") for _ in range(C)] for k in "abc"}
                outs_d = [[torch.zeros(cap1 // 4, dtype=torch.int32, device="cuda") for _ in range(C)] for _ in range(n)]
                dec = {k: torch.empty_like(fr) for k in "abcd"}

                def enc_a():
                    return ctx.encode_eg_frames_vq_dev(fr, W, H, C, n, pal, const, outs["a"], [cap] * C)

                def enc_b():
                    return ctx_q.encode_eg_frames_dev(fr, W, H, C, n, outs["b"], [cap] * C)

                def enc_c():
                    return ctx.encode_eg_frames_vq_dev(fr, W, H, C, n, pal, cyc, outs["c"], [cap] * C)

                def enc_d():
                    carry, totals = [(0, 0)] * C, []
                    for s in range(n):
                        tb = per_table[cyc[s]].encode_eg_frames_dev(fr[s * D:(s + 1) * D], W, H, C, 1, outs_d[s], [cap1] * C, carry)
                        totals.append(tb)
                        # the next stack continues the partial byte: one byte per channel read back
                        carry = [(int(outs_d[s][ch].view(torch.uint8)[t // 8].item()) if t % 8 else 0, t % 8)
                                 for ch, t in enumerate(tb)]
                    return totals

                tb_a, tb_b, tb_c, tb_d = enc_a(), enc_b(), enc_c(), enc_d()
                stream.synchronize()
                host = {k: [o.cpu().numpy().view(np.uint8) for o in outs[k]] for k in "abc"}
                same_ab = tb_a == tb_b and all(np.array_equal(host["a"][ch][:(tb_a[ch] + 7) // 8], host["b"][ch][:(tb_b[ch] + 7) // 8])
                                              for ch in range(C))
                # (d)'s stacks against (c)'s stream: stack s's bytes begin inside the byte its carry came from
                same_cd = True
                for ch in range(C):
                    pos = 0
                    for s in range(n):
                        t = tb_d[s][ch]
                        got = outs_d[s][ch].cpu().numpy().view(np.uint8)[:(t + 7) // 8]
                        want = host["c"][ch][pos // 8:pos // 8 + (t + 7) // 8].copy()
                        if t % 8:  # the bits behind this stack's end belong to the next stack
                            want[-1] &= (0xFF00 >> (t % 8)) & 0xFF
                        same_cd = same_cd and np.array_equal(got, want)
                        pos = pos // 8 * 8 + t
                    same_cd = same_cd and pos == tb_c[ch]
                nbytes = {k: [(t + 7) // 8 for t in tb] for k, tb in (("a", tb_a), ("c", tb_c))}

                def dec_a():
                    return ctx.decode_eg_frames_vq_dev(outs["a"], nbytes["a"], [0] * C, W, H, n, pal, const, dec["a"])

                def dec_b():
                    return ctx_q.decode_eg_frames_dev(outs["a"], nbytes["a"], [0] * C, W, H, n, dec["b"])

                def dec_c():
                    return ctx.decode_eg_frames_vq_dev(outs["c"], nbytes["c"], [0] * C, W, H, n, pal, cyc, dec["c"])

                def dec_d():
                    pos = [0] * C
                    for s in range(n):  # each call starts where the one before ended (a 4-byte aligned word, a bit in it)
                        ptrs = [outs["c"][ch].data_ptr() + pos[ch] // 32 * 4 for ch in range(C)]
                        eb = per_table[cyc[s]].decode_eg_frames_dev(ptrs, [nbytes["c"][ch] - pos[ch] // 32 * 4 for ch in range(C)],
                                                                     [p % 32 for p in pos], W, H, 1, dec["d"][s * D:(s + 1) * D])
                        pos = [p // 32 * 32 + e for p, e in zip(pos, eb)]
                    return pos

                eb_a, eb_b, eb_c, eb_d = dec_a(), dec_b(), dec_c(), dec_d()
                stream.synchronize()
                same_ab = same_ab and eb_a == eb_b == tb_a and bool(torch.equal(dec["a"], dec["b"]))
                same_cd = same_cd and eb_c == eb_d == tb_c and bool(torch.equal(dec["c"], dec["d"]))
                cfg = {"depth": D, "channels": C, "a_equals_b": bool(same_ab), "c_equals_d": bool(same_cd),
                       "bits_per_pixel": {"constant_q5": round(sum(tb_a) / (fr.numel() / C), 4),
                                          "cycling": round(sum(tb_c) / (fr.numel() / C), 4)}}
                for name, variants in (("encode", {"a_vq_constant": enc_a, "b_qt1": enc_b, "c_vq_cycling": enc_c, "d_contexts_chain": enc_d}),
                                       ("decode", {"a_vq_constant": dec_a, "b_qt1": dec_b, "c_vq_cycling": dec_c, "d_contexts_chain": dec_d})):
                    rounds = run_rounds(variants)
                    med = {k: statistics.median(v) for k, v in rounds.items()}
                    below = all(x < y for x, y in zip(rounds["c_vq_cycling"], rounds["d_contexts_chain"]))
                    ok = ok and below
                    cfg[name] = {"ms_per_round": rounds, "ms_median": med, "a_over_b": round(med["a_vq_constant"] / med["b_qt1"], 4),
                                 "c_over_d": round(med["c_vq_cycling"] / med["d_contexts_chain"], 4),
                                 "c_below_d_every_round": bool(below),
                                 "b_spread": round((max(rounds["b_qt1"]) - min(rounds["b_qt1"])) / med["b_qt1"], 4)}
                ok = ok and same_ab and same_cd
                res["configs"].append(cfg)
                for c in per_table + [ctx, ctx_q]:
                    c.close()
                del fr, outs, outs_d, dec
                torch.cuda.empty_cache()

    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    if not ok:
        raise SystemExit("the vq call is not below the chain of prepared contexts in every round, or its outputs differ")


if __name__ == "__main__":
    main()
