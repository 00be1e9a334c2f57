#!/usr/bin/env python3
"""Quantiser tables (dct3d_ctx_set_quant): what the table costs and what it buys, on device-resident 1920 x 1080
stacks (bench.py, the flagship measurement, is not involved).

  (a) the table kernels with the REFERENCE table (DCT3D_OPT_QUANT_FORCE_TABLE = 1)
  (b) the product kernels on the same buffers -- the yardstick: the outputs are identical (checked, bit for bit,
      before timing), so (a) / (b) is the pure cost of reading the steps from a table
  (c) quant_table(12) and (d) quant_table(1), on ramp and on uniform content: time per call, stream bytes, the
      exact paths' counts from stats() and the PSNR of the decoded frames against the input -- the
      rate-distortion and cost table of the knob, and where a flood of small-step rechecks would show

Calls: the int32 encode and decode (encode_frames_dev / decode_frames_dev) and the fused stream encode and decode
(encode_eg_frames_dev / decode_eg_frames_dev).  (a) / (b): grey (126 stacks) and packed RGB24 (42 stacks) at
8x8x8; (c) / (d): grey, at each of --depths.  Everything runs on one stream shared by torch and the context,
timed with device events; each variant is warmed up, then `--rounds` rounds alternate the variants, `--iters`
timed calls each, the round's figure being the median.  Prints one JSON document; --out also writes it to a file.

  --only enc|dec|eg_enc|eg_dec   for a profiler run of its own: untimed, `--iters` calls of (a) and then of (b)
                                 of that call on the first --channels entry
"""
import argparse
import importlib
import json
import math
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--channels", default="1,3")
    ap.add_argument("--grey-stacks", type=int, default=126)
    ap.add_argument("--rgb-stacks", type=int, default=42)
    ap.add_argument("--depths", default="8,4", help="block depths of the (c) / (d) table")
    ap.add_argument("--qualities", default="12,1")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default=None, choices=("enc", "dec", "eg_enc", "eg_dec"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    W, H = (int(v) for v in a.size.split("x"))

    import torch
    pkg = importlib.import_module("3ddctvideoencoding_amd")
    if not torch.cuda.is_available():
        raise SystemExit("bench_quant.py needs a HIP device")
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

    def content(ctx, D, C, n, kind):
        F = n * D
        if C == 1:
            t = torch.empty((F, H, W), dtype=torch.uint8, device="cuda")
            ctx.fill_synthetic_dev(t, W, H, F, kind=kind)
            return t
        planes = torch.empty((3, F, H, W), dtype=torch.uint8, device="cuda")
        ctx.fill_synthetic_dev(planes[0], W, H, F, kind=kind)
        ctx.fill_synthetic_dev(planes[1], W, H, F, seed=0x77A1, frame0=3, kind="uniform")
        ctx.fill_synthetic_dev(planes[2], W, H, F, seed=0x51DE5, frame0=11, kind=kind)
        return planes.permute(1, 2, 3, 0).contiguous()

    class Clip:
        """one clip's device buffers and the four calls on them"""

        def __init__(self, ctx, D, C, n, kind):
            self.ctx, self.D, self.C, self.n = ctx, D, C, n
            self.fr = content(ctx, D, C, n, kind)
            Wp, Hp = pkg.padded_size(W, H)
            self.q = torch.empty((C * ctx.n_cubes(Wp, Hp, n), D, 8, 8), dtype=torch.int32, device="cuda")
            self.out = torch.empty_like(self.fr)
            self.cap = (self.fr.numel() // C * 3 + 64) // 4 * 4  # bytes per channel's stream (24 bits a value)
            self.streams = [torch.zeros(self.cap // 4, dtype=torch.int32, device="cuda") for _ in range(C)]
            self.bits = [0] * C

        def enc(self):
            self.ctx.encode_frames_dev(self.fr, W, H, self.C, self.n, self.q)

        def dec(self):
            self.ctx.decode_frames_dev(self.q, W, H, self.C, self.n, self.out)

        def eg_enc(self):
            self.bits = self.ctx.encode_eg_frames_dev(self.fr, W, H, self.C, self.n, self.streams, [self.cap] * self.C)

        def eg_dec(self):
            self.ctx.decode_eg_frames_dev(self.streams, [(b + 7) // 8 for b in self.bits], [0] * self.C, W, H, self.n,
                                          self.out)

        def snapshot(self):
            """(q, frames from q, stream bytes, frames from the streams) of the current table / option"""
            self.enc()
            q = self.q.clone()
            self.dec()
            o = self.out.clone()
            self.eg_enc()
            s = [t[: (b + 31) // 32].clone() for t, b in zip(self.streams, self.bits)]
            self.eg_dec()
            return q, o, s, self.out.clone(), list(self.bits)

    CALLS = ("enc", "dec", "eg_enc", "eg_dec")
    res = {"tool": "bench_quant", "size": a.size, "iters": a.iters, "rounds": a.rounds, "table_cost": [], "tables": []}

    with torch.cuda.stream(stream):
        # ---- (a) / (b): the cost of the table, 8x8x8 ----
        ctx = pkg.Context(0, 8, 8, 8)
        ctx.set_stream(stream.cuda_stream)
        for C in (int(c) for c in a.channels.split(",")):
            n = a.grey_stacks if C == 1 else a.rgb_stacks
            clip = Clip(ctx, 8, C, n, "ramp")

            def variant(call, force):
                def fn():
                    ctx.set_option(pkg.DCT3D_OPT_QUANT_FORCE_TABLE, force)
                    getattr(clip, call)()
                return fn

            if a.only:
                clip.enc()
                clip.eg_enc()
                for force in (1, 0):
                    for _ in range(a.iters):
                        variant(a.only, force)()
                stream.synchronize()
                print(json.dumps({"only": a.only, "channels": C, "stacks": n, "iters": a.iters, "order": "table, product"}))
                ctx.close()
                return
            ctx.set_option(pkg.DCT3D_OPT_QUANT_FORCE_TABLE, 1)
            sa = clip.snapshot()
            ctx.set_option(pkg.DCT3D_OPT_QUANT_FORCE_TABLE, 0)
            sb = clip.snapshot()
            same = (torch.equal(sa[0], sb[0]) and torch.equal(sa[1], sb[1]) and torch.equal(sa[3], sb[3]) and
                    sa[4] == sb[4] and all(torch.equal(x, y) for x, y in zip(sa[2], sb[2])))
            del sa, sb
            variants = {}
            for call in CALLS:
                variants[call + "_a_table"] = variant(call, 1)
                variants[call + "_b_product"] = variant(call, 0)
            rounds = run_rounds(variants)
            ctx.set_option(pkg.DCT3D_OPT_QUANT_FORCE_TABLE, 0)
            med = {k: statistics.median(v) for k, v in rounds.items()}
            res["table_cost"].append({
                "channels": C, "stacks": n, "depth": 8, "outputs_identical": bool(same), "ms_per_round": rounds,
                "ms_median": med,
                "a_over_b": {call: round(med[call + "_a_table"] / med[call + "_b_product"], 4) for call in CALLS},
                "b_spread": {call: round((max(rounds[call + "_b_product"]) - min(rounds[call + "_b_product"])) /
                                         med[call + "_b_product"], 4) for call in CALLS}})
            del clip
            torch.cuda.empty_cache()
        ctx.close()

        # ---- (c) / (d): what the knob buys, grey ----
        for D in (int(d) for d in a.depths.split(",")):
            ctx = pkg.Context(0, 8, 8, D)
            ctx.set_stream(stream.cuda_stream)
            n = a.grey_stacks
            for kind in ("ramp", "uniform"):
                clip = Clip(ctx, D, 1, n, kind)
                for quality in [5] + [int(v) for v in a.qualities.split(",")]:
                    ctx.set_quant(None if quality == 5 else pkg.quant_table(quality, D))
                    stats = {}
                    for call in CALLS:  # in this order: the decodes take the encodes' outputs
                        getattr(clip, call)()
                        st = ctx.stats()
                        stats[call] = {"n_units": st["n_units"], "n_flagged": st["n_flagged"], "n_rechecked": st["n_rechecked"]}
                    mse = float(((clip.out.float() - clip.fr.float()) ** 2).mean().item())
                    rounds = run_rounds({call: getattr(clip, call) for call in CALLS})
                    res["tables"].append({
                        "depth": D, "content": kind, "stacks": n, "table": f"quant_table({quality})",
                        "reference_table": quality == 5, "input_bytes": clip.fr.numel(),
                        "stream_bytes": (clip.bits[0] + 7) // 8,
                        "bits_per_pixel": round(clip.bits[0] / clip.fr.numel(), 4),
                        "psnr_db": round(10 * math.log10(255.0 ** 2 / mse), 3) if mse > 0 else None,
                        "exact_paths": stats, "ms_per_round": rounds,
                        "ms_median": {k: statistics.median(v) for k, v in rounds.items()}})
                del clip
                torch.cuda.empty_cache()
            ctx.close()

    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    if not all(c["outputs_identical"] for c in res["table_cost"]):
        raise SystemExit("the table kernels with the reference table and the product kernels differ")


if __name__ == "__main__":
    main()
