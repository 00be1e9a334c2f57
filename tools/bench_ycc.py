#!/usr/bin/env python3
"""The YCbCr colour transform fused into the packed RGB24 stream calls (DCT3D_OPT_COLOUR) against what a
caller had before it, on device-resident 1080p stacks (bench.py, the flagship measurement, is not involved).

Per direction:
  (a) the option on: frames -> the Y, Cb, Cr streams, and those streams -> RGB frames
  (b) the option off on the same bytes: the same kernels without the colour arm, i.e. the ceiling
  (c) what a caller of the parent commit can do: a torch integer transform into a second raster, then the option-off
      call (encode), and the option-off call followed by the torch inverse into a second raster (decode)
Before timing, (c)'s streams and frames are compared with (a)'s, bit for bit.

Content: 42 packed RGB24 stacks of 1920 x 1080, ramp and uniform (three dct3d_fill_synthetic_dev planes of different
seeds, interleaved: bench_eg_frames.py's), 8 x 8 x 8 or --depth 4.  Everything runs on one stream shared by torch and
the contexts, timed with device events; each case is warmed up, then `--rounds` rounds alternate the variants,
`--iters` timed calls each, the round's figure being the median.  Also records the rate probe's bits with the option
on and off under the reference table and quant_table(12): synthetic content, so an illustration and no claim about
video.  Prints one JSON document; --out also writes it to a file.

  --only enc|dec   for a profiler run of its own: untimed, `--iters` calls of (a) (or, with --off, of (b)) of the
                   first --kinds entry
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
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--kinds", default="ramp,uniform")
    ap.add_argument("--stacks", type=int, default=42)
    ap.add_argument("--depth", type=int, default=8, choices=(8, 4))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default=None, choices=("enc", "dec"))
    ap.add_argument("--off", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    pkg = importlib.import_module("3ddctvideoencoding_amd")
    if not torch.cuda.is_available():
        raise SystemExit("bench_ycc.py needs a HIP device")
    D, n = a.depth, a.stacks
    cs = 64 * D
    W, H = (int(v) for v in a.size.split("x"))
    Wp, Hp = pkg.padded_size(W, H)
    stream = torch.cuda.Stream()
    ctx_on, ctx_off = pkg.Context(0, 8, 8, D), pkg.Context(0, 8, 8, D)
    for c in (ctx_on, ctx_off):
        c.set_stream(stream.cuda_stream)
    ctx_on.set_option(pkg.DCT3D_OPT_COLOUR, pkg.DCT3D_COLOUR_YCBCR)

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

    def content(kind):
        F = n * D
        planes = torch.empty((3, F, H, W), dtype=torch.uint8, device="cuda")
        ctx_off.fill_synthetic_dev(planes[0], W, H, F, kind=kind)
        ctx_off.fill_synthetic_dev(planes[1], W, H, F, seed=0x77A1, frame0=3, kind=kind)
        ctx_off.fill_synthetic_dev(planes[2], W, H, F, seed=0x51DE5, frame0=11, kind=kind)
        return planes.permute(1, 2, 3, 0).contiguous()

    # the definition (rgb_to_ycbcr / ycbcr_to_rgb) in torch integers, one stack at a time into a second raster (the
    # int32 temporaries of the whole clip would be 12 x its size)
    def t_forward(src, dst):
        for s in range(n):
            x = src[s * D:(s + 1) * D].to(torch.int32)
            r, g, b = x[..., 0], x[..., 1], x[..., 2]
            o = dst[s * D:(s + 1) * D]
            o[..., 0] = ((19595 * r + 38470 * g + 7471 * b + 32768) >> 16).to(torch.uint8)
            o[..., 1] = ((-11059 * r - 21709 * g + 32768 * b + ((128 << 16) + 32767)) >> 16).to(torch.uint8)
            o[..., 2] = ((32768 * r - 27439 * g - 5329 * b + ((128 << 16) + 32767)) >> 16).to(torch.uint8)

    def t_inverse(src, dst):
        for s in range(n):
            x = src[s * D:(s + 1) * D].to(torch.int32)
            y, u, v = x[..., 0], x[..., 1] - 128, x[..., 2] - 128
            o = dst[s * D:(s + 1) * D]
            o[..., 0] = (y + ((91881 * v + 32768) >> 16)).clamp_(0, 255).to(torch.uint8)
            o[..., 1] = (y + ((-22554 * u - 46802 * v + 32768) >> 16)).clamp_(0, 255).to(torch.uint8)
            o[..., 2] = (y + ((116130 * u + 32768) >> 16)).clamp_(0, 255).to(torch.uint8)

    cases = []
    with torch.cuda.stream(stream):
        for kind in a.kinds.split(","):
            n_cubes = ctx_on.n_cubes(Wp, Hp, n)  # per channel
            d_fr = content(kind)
            d_t = torch.empty_like(d_fr)        # (c): the transformed raster
            cap = n_cubes * cs + 64             # bytes per channel: 8 bits per value
            d_s = {k: [torch.zeros(cap // 4 + 1, dtype=torch.int32, device="cuda") for _ in range(3)] for k in "abc"}
            d_out = {k: torch.empty_like(d_fr) for k in "abc"}
            d_tmp = torch.empty_like(d_fr)      # (c): the decoded Y, Cb, Cr raster
            bits = {}

            def enc_a():
                bits["a"] = ctx_on.encode_eg_frames_dev(d_fr, W, H, 3, n, d_s["a"], [cap] * 3)

            def enc_b():
                bits["b"] = ctx_off.encode_eg_frames_dev(d_fr, W, H, 3, n, d_s["b"], [cap] * 3)

            def enc_c():
                t_forward(d_fr, d_t)
                bits["c"] = ctx_off.encode_eg_frames_dev(d_t, W, H, 3, n, d_s["c"], [cap] * 3)

            def nbytes():
                return [(b + 7) // 8 for b in bits["a"]]

            def dec_a():
                ctx_on.decode_eg_frames_dev(d_s["a"], nbytes(), [0] * 3, W, H, n, d_out["a"])

            def dec_b():
                ctx_off.decode_eg_frames_dev(d_s["a"], nbytes(), [0] * 3, W, H, n, d_out["b"])

            def dec_c():
                ctx_off.decode_eg_frames_dev(d_s["a"], nbytes(), [0] * 3, W, H, n, d_tmp)
                t_inverse(d_tmp, d_out["c"])

            if a.only:
                enc_a()
                fn = {"enc": enc_b if a.off else enc_a, "dec": dec_b if a.off else dec_a}[a.only]
                for _ in range(a.iters):
                    fn()
                stream.synchronize()
                print(json.dumps({"only": a.only, "option": "off" if a.off else "on", "size": a.size, "kind": kind, "stacks": n,
                                  "calls": a.iters, "frame_bytes": d_fr.numel(), "stream_bytes": nbytes()}))
                ctx_on.close()
                ctx_off.close()
                return
            enc_a()
            enc_c()
            dec_a()
            dec_c()
            stream.synchronize()
            equal = bits["a"] == bits["c"] and bool(torch.equal(d_out["a"], d_out["c"])) and all(
                bool(torch.equal(x[:(b + 31) // 32], y[:(b + 31) // 32])) for x, y, b in zip(d_s["a"], d_s["c"], bits["a"]))
            rounds = run_rounds({"enc_a_on": enc_a, "enc_b_off_same_bytes": enc_b, "enc_c_torch_then_off": enc_c,
                                 "dec_a_on": dec_a, "dec_b_off_same_streams": dec_b, "dec_c_off_then_torch": dec_c})
            med = {k: statistics.median(v) for k, v in rounds.items()}

            def kernel_split(ctx, fn):
                """per call, from the context's own event pairs: the transform kernels and the auxiliary launches"""
                stream.synchronize()
                ctx.reset_timers()
                ctx.set_profiling(True)
                for _ in range(a.iters):
                    fn()
                st = ctx.stats()
                ctx.set_profiling(False)
                return {"kernel_ms": round(st["kernel_ms_total"] / a.iters, 4), "aux_ms": round(st["aux_ms_total"] / a.iters, 4)}

            split = {k: kernel_split(c, fn) for k, c, fn in (("enc_a_on", ctx_on, enc_a), ("enc_b_off_same_bytes", ctx_off, enc_b),
                                                             ("dec_a_on", ctx_on, dec_a), ("dec_b_off_same_streams", ctx_off, dec_b))}
            tabs = [pkg.quant_table(5, D), pkg.quant_table(12, D)]
            rate = {k: c.rate_frames_dev(d_fr, W, H, 3, n, tabs).sum(axis=1).tolist() for k, c in (("on", ctx_on), ("off", ctx_off))}
            cases.append({
                "size": a.size, "kind": kind, "stacks": n, "frame_bytes": d_fr.numel(), "stream_bits_on": bits["a"],
                "stream_bits_off": bits["b"], "ms_per_round": rounds, "ms_median": med, "kernel_split_per_call": split,
                "enc_a_over_b": round(med["enc_a_on"] / med["enc_b_off_same_bytes"], 4),
                "enc_a_over_c": round(med["enc_a_on"] / med["enc_c_torch_then_off"], 4),
                "dec_a_over_b": round(med["dec_a_on"] / med["dec_b_off_same_streams"], 4),
                "dec_a_over_c": round(med["dec_a_on"] / med["dec_c_off_then_torch"], 4),
                "enc_a_faster_than_c_every_round": all(x < y for x, y in zip(rounds["enc_a_on"], rounds["enc_c_torch_then_off"])),
                "dec_a_faster_than_c_every_round": all(x < y for x, y in zip(rounds["dec_a_on"], rounds["dec_c_off_then_torch"])),
                "a_equals_c": equal,
                # [table: reference, quant_table(12)][channel: Y Cb Cr | R G B], summed over the stacks
                "rate_bits": rate,
                "rate_on_over_off": [round(sum(rate["on"][t]) / sum(rate["off"][t]), 4) for t in range(2)],
            })
            del d_fr, d_t, d_s, d_out, d_tmp
            torch.cuda.empty_cache()

    res = {"tool": "bench_ycc", "depth": D, "iters": a.iters, "rounds": a.rounds,
           "content": "three dct3d_fill_synthetic_dev planes (default seed; seed 0x77A1, frame0 3; seed 0x51DE5, frame0 11), interleaved",
           "cases": cases}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    ctx_on.close()
    ctx_off.close()
    if not all(c["a_equals_c"] for c in cases):
        raise SystemExit("the option's results and the torch transform's differ")


if __name__ == "__main__":
    main()
