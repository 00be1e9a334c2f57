#!/usr/bin/env python3
"""4:2:0 chroma subsampling fused into the YCbCr stream calls (dct3d_ctx_set_chroma) against the 4:4:4
calls and against what a caller had before it, on device-resident 1080p stacks (bench.py, the flagship measurement,
is not involved).

Per direction:
  (a) 4:2:0 on: frames -> the Y, S(Cb), S(Cr) streams, and those streams -> RGB frames
  (b) the colour transform at 4:4:4 on the same frames (and, for the decode, on its own streams): three full planes
  (c) what a caller of the parent commit can do: a torch integer transform and 2 x 2 box mean into three planes plus
      three grey stream calls (encode), and three grey stream calls plus a torch replication and inverse transform into
      the frames (decode).  (c)'s streams and frames equal (a)'s, bit for bit (checked before timing).

Content: 42 packed RGB24 stacks of 1920 x 1080, ramp and uniform (three dct3d_fill_synthetic_dev planes of different
seeds, interleaved: bench_ycc.py's), 8 x 8 x 8 or --depth 4.  Everything runs on one stream shared by torch and the
contexts, timed with device events; each case is warmed up, then `--rounds` rounds alternate the variants, `--iters`
timed calls each, the round's figure being the median.  Also records the rate probe's bits at 4:2:0 and 4:4:4 under the
reference table and quant_table(12): synthetic content, so an illustration and no claim about video.  Prints one JSON
document; --out also writes it to a file.

  --only enc|dec   for a profiler run of its own: untimed, `--iters` calls of (a) (or, with --b444, of (b)) of the
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
    ap.add_argument("--b444", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    pkg = importlib.import_module("3ddctvideoencoding_amd")
    if not torch.cuda.is_available():
        raise SystemExit("bench_c420.py needs a HIP device")
    D, n = a.depth, a.stacks
    cs = 64 * D
    W, H = (int(v) for v in a.size.split("x"))
    CW, CH = pkg.chroma_size(W, H)
    sizes = [(W, H), (CW, CH), (CW, CH)]
    stream = torch.cuda.Stream()
    ctx_420, ctx_444, ctx_grey = (pkg.Context(0, 8, 8, D) for _ in range(3))
    for c in (ctx_420, ctx_444, ctx_grey):
        c.set_stream(stream.cuda_stream)
    for c in (ctx_420, ctx_444):
        c.set_option(pkg.DCT3D_OPT_COLOUR, pkg.DCT3D_COLOUR_YCBCR)
    ctx_420.set_chroma(pkg.DCT3D_CHROMA_420)

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
        ctx_grey.fill_synthetic_dev(planes[0], W, H, F, kind=kind)
        ctx_grey.fill_synthetic_dev(planes[1], W, H, F, seed=0x77A1, frame0=3, kind=kind)
        ctx_grey.fill_synthetic_dev(planes[2], W, H, F, seed=0x51DE5, frame0=11, kind=kind)
        return planes.permute(1, 2, 3, 0).contiguous()

    # the definitions (rgb_to_ycbcr420 / ycbcr420_to_rgb) in torch integers, one stack at a time
    def box(p):
        if W % 2:
            p = torch.cat((p, p[:, :, -1:]), dim=2)
        if H % 2:
            p = torch.cat((p, p[:, -1:, :]), dim=1)
        return ((p[:, 0::2, 0::2] + p[:, 0::2, 1::2] + p[:, 1::2, 0::2] + p[:, 1::2, 1::2] + 2) >> 2).to(torch.uint8)

    def t_forward(src, planes):
        for s in range(n):
            x = src[s * D:(s + 1) * D].to(torch.int32)
            r, g, b = x[..., 0], x[..., 1], x[..., 2]
            sl = slice(s * D, (s + 1) * D)
            planes[0][sl] = ((19595 * r + 38470 * g + 7471 * b + 32768) >> 16).to(torch.uint8)
            planes[1][sl] = box((-11059 * r - 21709 * g + 32768 * b + ((128 << 16) + 32767)) >> 16)
            planes[2][sl] = box((32768 * r - 27439 * g - 5329 * b + ((128 << 16) + 32767)) >> 16)

    def up(c):
        return c.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)[:, :H, :W].to(torch.int32)

    def t_inverse(planes, dst):
        for s in range(n):
            sl = slice(s * D, (s + 1) * D)
            y, u, v = planes[0][sl].to(torch.int32), up(planes[1][sl]) - 128, up(planes[2][sl]) - 128
            o = dst[sl]
            o[..., 0] = (y + ((91881 * v + 32768) >> 16)).clamp_(0, 255).to(torch.uint8)
            o[..., 1] = (y + ((-22554 * u - 46802 * v + 32768) >> 16)).clamp_(0, 255).to(torch.uint8)
            o[..., 2] = (y + ((116130 * u + 32768) >> 16)).clamp_(0, 255).to(torch.uint8)

    cases = []
    with torch.cuda.stream(stream):
        for kind in a.kinds.split(","):
            d_fr = content(kind)
            caps = [(-(-w // 8)) * (-(-h // 8)) * n * cs + 64 for w, h in sizes]  # bytes per stream: 8 bits per value
            d_s = {k: [torch.zeros((caps[0] if k == "b" else c) // 4 + 1, dtype=torch.int32, device="cuda") for c in caps] for k in "abc"}
            d_out = {k: torch.empty_like(d_fr) for k in "abc"}
            d_pl = [torch.empty((n * D, h, w), dtype=torch.uint8, device="cuda") for w, h in sizes]   # (c): encode side
            d_dec = [torch.empty((n * D, h, w), dtype=torch.uint8, device="cuda") for w, h in sizes]  # (c): decode side
            bits = {}

            def enc_a():
                bits["a"] = ctx_420.encode_eg_frames_dev(d_fr, W, H, 3, n, d_s["a"], caps)

            def enc_b():
                bits["b"] = ctx_444.encode_eg_frames_dev(d_fr, W, H, 3, n, d_s["b"], [caps[0]] * 3)

            def enc_c():
                t_forward(d_fr, d_pl)
                bits["c"] = [ctx_grey.encode_eg_frames_dev(d_pl[k], sizes[k][0], sizes[k][1], 1, n, [d_s["c"][k]], [caps[k]])[0]
                             for k in range(3)]

            def nbytes(k):
                return [(b + 7) // 8 for b in bits[k]]

            def dec_a():
                ctx_420.decode_eg_frames_dev(d_s["a"], nbytes("a"), [0] * 3, W, H, n, d_out["a"])

            def dec_b():
                ctx_444.decode_eg_frames_dev(d_s["b"], nbytes("b"), [0] * 3, W, H, n, d_out["b"])

            def dec_c():
                for k in range(3):
                    ctx_grey.decode_eg_frames_dev([d_s["a"][k]], [nbytes("a")[k]], [0], sizes[k][0], sizes[k][1], n, d_dec[k])
                t_inverse(d_dec, d_out["c"])

            enc_a()
            enc_b()
            if a.only:
                fn = {"enc": enc_b if a.b444 else enc_a, "dec": dec_b if a.b444 else dec_a}[a.only]
                for _ in range(a.iters):
                    fn()
                stream.synchronize()
                print(json.dumps({"only": a.only, "chroma": "444" if a.b444 else "420", "size": a.size, "kind": kind, "stacks": n,
                                  "calls": a.iters, "frame_bytes": d_fr.numel(), "stream_bytes": nbytes("b" if a.b444 else "a")}))
                for c in (ctx_420, ctx_444, ctx_grey):
                    c.close()
                return
            enc_c()
            dec_a()
            dec_c()
            stream.synchronize()
            equal = bits["a"] == bits["c"] and bool(torch.equal(d_out["a"], d_out["c"])) and all(
                bool(torch.equal(x[:(b + 31) // 32], y[:(b + 31) // 32])) for x, y, b in zip(d_s["a"], d_s["c"], bits["a"]))
            rounds = run_rounds({"enc_a_420": enc_a, "enc_b_444": enc_b, "enc_c_torch_then_grey": enc_c,
                                 "dec_a_420": dec_a, "dec_b_444": dec_b, "dec_c_grey_then_torch": dec_c})
            med = {k: statistics.median(v) for k, v in rounds.items()}
            tabs = [pkg.quant_table(5, D), pkg.quant_table(12, D)]
            rate = {k: c.rate_frames_dev(d_fr, W, H, 3, n, tabs).sum(axis=1).tolist() for k, c in (("420", ctx_420), ("444", ctx_444))}
            cases.append({
                "size": a.size, "kind": kind, "stacks": n, "frame_bytes": d_fr.numel(), "stream_bits_420": bits["a"],
                "stream_bits_444": bits["b"], "ms_per_round": rounds, "ms_median": med,
                "enc_a_over_b": round(med["enc_a_420"] / med["enc_b_444"], 4),
                "enc_a_over_c": round(med["enc_a_420"] / med["enc_c_torch_then_grey"], 4),
                "dec_a_over_b": round(med["dec_a_420"] / med["dec_b_444"], 4),
                "dec_a_over_c": round(med["dec_a_420"] / med["dec_c_grey_then_torch"], 4),
                "enc_a_faster_than_c_every_round": all(x < y for x, y in zip(rounds["enc_a_420"], rounds["enc_c_torch_then_grey"])),
                "dec_a_faster_than_c_every_round": all(x < y for x, y in zip(rounds["dec_a_420"], rounds["dec_c_grey_then_torch"])),
                "a_equals_c": equal,
                # [table: reference, quant_table(12)][channel: Y Cb Cr], summed over the stacks
                "rate_bits": rate,
                "rate_420_over_444": [round(sum(rate["420"][t]) / sum(rate["444"][t]), 4) for t in range(2)],
            })
            del d_fr, d_s, d_out, d_pl, d_dec
            torch.cuda.empty_cache()

    res = {"tool": "bench_c420", "depth": D, "iters": a.iters, "rounds": a.rounds,
           "content": "three dct3d_fill_synthetic_dev planes (default seed; seed 0x77A1, frame0 3; seed 0x51DE5, frame0 11), interleaved",
           "cases": cases}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    for c in (ctx_420, ctx_444, ctx_grey):
        c.close()
    if not all(c["a_equals_c"] for c in cases):
        raise SystemExit("the 4:2:0 calls' results and the torch route's differ")


if __name__ == "__main__":
    main()
