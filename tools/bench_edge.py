#!/usr/bin/env python3
"""Frames of any size (encode_frames_dev / decode_frames_dev) against what a caller could do without them, on
device-resident stacks of common screen sizes (bench.py, the flagship measurement, is not involved).

  (a) the new call on the unpadded frames
  (b) the caller's way on the parent commit: encode = a replicate-padded copy (torch) + the existing call at the
      padded size; decode = the existing call into a padded raster + a cropping .contiguous() copy
  (c) the existing call on content of the padded size alone: the ceiling
  (d) at 1920 x 1080 (multiples of 8): the new call against the existing call -- the same kernel; "inside the
      spread": the two medians differ by no more than the existing call's own max - min over the rounds

Grey (126 stacks) and packed RGB24 (42 stacks).  Everything runs on one stream shared by torch and the context,
timed with device events; each case is warmed up, then `--rounds` rounds alternate the variants, `--iters`
timed calls each, the round's figure being the median.  Before timing, (a) is compared with (b), bit for bit,
at the timed size.  Prints one JSON document; --out also writes it to a file.

  --only enc|dec   for a profiler run of its own: untimed, `--iters` calls of (a) and then of (c) of the first
                   --sizes entry and the first --channels entry
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
    ap.add_argument("--sizes", default="1366x768,1600x900,1680x1050")
    ap.add_argument("--channels", default="1,3")
    ap.add_argument("--grey-stacks", type=int, default=126)
    ap.add_argument("--rgb-stacks", type=int, default=42)
    ap.add_argument("--depth", type=int, default=8, choices=(8, 4))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default=None, choices=("enc", "dec"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    pkg = importlib.import_module("3ddctvideoencoding_amd")
    if not torch.cuda.is_available():
        raise SystemExit("bench_edge.py needs a HIP device")
    D = a.depth
    stream = torch.cuda.Stream()
    ctx = pkg.Context(0, 8, 8, D)
    ctx.set_stream(stream.cuda_stream)

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

    def content(W, H, C, n):
        """padded-size content [F, Hp, Wp(, 3)] (ramp; RGB: ramp, uniform, ramp), device resident"""
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

    def existing_enc(x, W, H, C, n, q):
        (ctx.encode_stacks_dev if C == 1 else ctx.encode_stacks_rgb_dev)(x, W, H, n, q)

    def existing_dec(q, W, H, C, n, x):
        (ctx.decode_stacks_dev if C == 1 else ctx.decode_stacks_rgb_dev)(q, W, H, n, x)

    def pad_replicate(x, Hp, Wp, out):
        """what a caller has: a padded copy with the last column and row repeated (grey: one torch pad kernel;
        packed RGB: the interior copy and two edge fills -- replicate padding acts on the last dimensions only)"""
        H, W = x.shape[1:3]
        if x.dim() == 3 and grey_pad != "slice copies":
            out.copy_(torch.nn.functional.pad(x.unsqueeze(0), (0, Wp - W, 0, Hp - H), mode="replicate")[0])
        else:
            out[:, :H, :W] = x
            if Wp > W:
                out[:, :H, W:] = x[:, :, W - 1:W]
            if Hp > H:
                out[:, H:] = out[:, H - 1:H]

    cases = []
    with torch.cuda.stream(stream):
        try:  # (replicate padding of bytes, if this torch has it; else the slice copies for grey too)
            torch.nn.functional.pad(torch.zeros((1, 2, 3, 3), dtype=torch.uint8, device="cuda"), (0, 1, 0, 1), mode="replicate")
            grey_pad = "torch.nn.functional.pad(mode='replicate')"
        except Exception:  # noqa: BLE001
            grey_pad = "slice copies"
        for size in a.sizes.split(","):
            W, H = (int(v) for v in size.split("x"))
            Wp, Hp = pkg.padded_size(W, H)
            for C in (int(c) for c in a.channels.split(",")):
                n = a.grey_stacks if C == 1 else a.rgb_stacks
                F = n * D
                d_pad = content(Wp, Hp, C, n)                       # (c)'s input, and the source of the frames
                d_fr = d_pad[:, :H, :W].contiguous()                # the unpadded frames
                pad_replicate(d_fr, Hp, Wp, d_pad)                  # now d_pad is their padded raster
                n_cubes = ctx.n_cubes(Wp, Hp, n)
                d_q = torch.empty((C * n_cubes, D, 8, 8), dtype=torch.int32, device="cuda")
                d_q2 = torch.empty_like(d_q)
                d_out = torch.empty_like(d_fr)
                d_out_pad = torch.empty_like(d_pad)
                d_tmp = torch.empty_like(d_pad)
                def enc_a():
                    ctx.encode_frames_dev(d_fr, W, H, C, n, d_q)

                def enc_b():
                    pad_replicate(d_fr, Hp, Wp, d_tmp)
                    existing_enc(d_tmp, Wp, Hp, C, n, d_q2)

                def enc_c():
                    existing_enc(d_pad, Wp, Hp, C, n, d_q2)

                def dec_a():
                    ctx.decode_frames_dev(d_q, W, H, C, n, d_out)

                def dec_b():
                    existing_dec(d_q, Wp, Hp, C, n, d_out_pad)
                    return d_out_pad[:, :H, :W].contiguous()

                def dec_c():
                    existing_dec(d_q, Wp, Hp, C, n, d_out_pad)

                if a.only:
                    enc_a()  # d_q for the decodes
                    for fn in ((enc_a, enc_c) if a.only == "enc" else (dec_a, dec_c)):
                        for _ in range(a.iters):
                            fn()
                    stream.synchronize()
                    print(json.dumps({"only": a.only, "size": size, "padded": f"{Wp}x{Hp}", "channels": C, "stacks": n,
                                      "iters": a.iters, "frame_bytes": d_fr.numel(), "padded_bytes": d_pad.numel()}))
                    ctx.close()
                    return
                enc_a()
                enc_b()
                enc_equal = bool(torch.equal(d_q, d_q2))
                dec_a()
                dec_equal = bool(torch.equal(d_out, dec_b()))
                rounds = run_rounds({"enc_a_new": enc_a, "enc_b_pad_copy": enc_b, "enc_c_ceiling": enc_c,
                                     "dec_a_new": dec_a, "dec_b_crop_copy": dec_b, "dec_c_ceiling": dec_c})
                med = {k: statistics.median(v) for k, v in rounds.items()}
                cases.append({
                    "size": size, "padded": f"{Wp}x{Hp}", "channels": C, "stacks": n,
                    "frame_bytes": d_fr.numel(), "padded_bytes": d_pad.numel(),
                    "ms_per_round": rounds, "ms_median": med,
                    "enc_a_over_b": round(med["enc_a_new"] / med["enc_b_pad_copy"], 4),
                    "enc_a_over_c": round(med["enc_a_new"] / med["enc_c_ceiling"], 4),
                    "dec_a_over_b": round(med["dec_a_new"] / med["dec_b_crop_copy"], 4),
                    "dec_a_over_c": round(med["dec_a_new"] / med["dec_c_ceiling"], 4),
                    "enc_a_faster_than_b_every_round": all(x < y for x, y in zip(rounds["enc_a_new"], rounds["enc_b_pad_copy"])),
                    "dec_a_faster_than_b_every_round": all(x < y for x, y in zip(rounds["dec_a_new"], rounds["dec_b_crop_copy"])),
                    "enc_a_equals_b": enc_equal, "dec_a_equals_b": dec_equal,
                })
                del d_pad, d_fr, d_q, d_q2, d_out, d_out_pad, d_tmp
                torch.cuda.empty_cache()

        # (d) multiples of 8: the new call is the existing call
        aligned = []
        W, H = 1920, 1080
        for C in (int(c) for c in a.channels.split(",")):
            n = a.grey_stacks if C == 1 else a.rgb_stacks
            d_fr = content(W, H, C, n)
            d_q = torch.empty((C * ctx.n_cubes(W, H, n), D, 8, 8), dtype=torch.int32, device="cuda")
            d_out = torch.empty_like(d_fr)
            rounds = run_rounds({
                "enc_new": lambda: ctx.encode_frames_dev(d_fr, W, H, C, n, d_q),
                "enc_existing": lambda: existing_enc(d_fr, W, H, C, n, d_q),
                "dec_new": lambda: ctx.decode_frames_dev(d_q, W, H, C, n, d_out),
                "dec_existing": lambda: existing_dec(d_q, W, H, C, n, d_out)})
            med = {k: statistics.median(v) for k, v in rounds.items()}

            def inside(new, old):
                """the two medians differ by no more than the existing call's own range over the rounds (max - min):
                the same kernel, so a difference is the run-to-run variation or it is not there"""
                return abs(med[new] - med[old]) <= max(rounds[old]) - min(rounds[old])

            aligned.append({"size": "1920x1080", "channels": C, "stacks": n, "ms_per_round": rounds, "ms_median": med,
                            "enc_new_over_existing": round(med["enc_new"] / med["enc_existing"], 4),
                            "dec_new_over_existing": round(med["dec_new"] / med["dec_existing"], 4),
                            "enc_new_inside_existing_spread": inside("enc_new", "enc_existing"),
                            "dec_new_inside_existing_spread": inside("dec_new", "dec_existing")})
            del d_fr, d_q, d_out
            torch.cuda.empty_cache()

    res = {"tool": "bench_edge", "depth": D, "iters": a.iters, "rounds": a.rounds, "grey_pad_method": grey_pad,
           "algorithmic_bytes_per_sample": {"new": 5, "copy_path": 7, "ceiling": 5},
           "cases": cases, "aligned_1920x1080": aligned}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    ctx.close()
    if not all(c["enc_a_equals_b"] and c["dec_a_equals_b"] for c in cases):
        raise SystemExit("the new calls and the copy path differ")


if __name__ == "__main__":
    main()
