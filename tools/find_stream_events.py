#!/usr/bin/env python3
"""Find (seed, pixel, sample, step) tuples whose generator step draws the ZERO WORD, and write tests/golden/stream_events.json.

A generator step (oracle/cpu_ref.cpp, "random streams") maps the stream's counter c to
    y = c ^ (c >> 16);   x = y * 0x7feb352d + k;   x ^= x >> 15;   the three draws are the top 24 bits of x * (M2, M2 A, M2 A^2)
For a fixed pixel key k this is a bijection of the 32-bit words, so exactly ONE counter gives x = 0 — the only x whose three draws
are all 0.0 (tests/test_rare_branches.py re-derives that from oracle.random).  Inverted:
    x = 0  <=>  y = -k * M1^-1 (mod 2^32)  <=>  c = y ^ (y >> 16)
and the counter of a stream stands at stride * position after `position` steps, position = (sample << 12) + step, so
    position = c * stride^-1 (mod 2^32).
One position in 2^32 per (seed, pixel).  The tuples worth keeping are those a small frame reaches: a small sample and
    step 1 of a sample > 0   the pixel jitter is exactly (0, 0)                                      kind "zero_jitter"
    step 2 of a sample > 0   random_unit_vector() draws (0, 0, 0) at the FIRST scatter and re-draws  kind "redraw_first_scatter"
    step 3 of a sample > 0   ... at the SECOND scatter (if the first took one step)                   kind "redraw_second_scatter"
    step 1 / 2 of sample 0   sample 0 draws no jitter: its first / second scatter                     kinds as above
About 3e-8 of the (seed, pixel) pairs qualify; the search below runs over whole blocks of seeds in numpy, a few million pairs per
second.  Recorded results only: the fixture holds no code.

--direct keeps steps 4 and 5 of a sample > 0 as well and writes tests/golden/stream_events_direct.json, a fixture of its own (the one
above is not regenerated).  Under RT_HIP_FLAG_DIRECT_LIGHT a lambert vertex draws a step k before its scatter's u, so
a sample's steps run jitter, k, u, k, u over two lambert vertices and jitter, u, k, u over a metal and a lambert one:
    step 4 of a sample > 0   kind "zero_word_step_4": the second scatter's u behind a metal first vertex (or the second vertex's k)
    step 5 of a sample > 0   kind "zero_word_step_5": the second scatter's u behind two lambert vertices
What such a word IS in a given scene is for the scene's census to say (tests/test_light_rare_branches.py)."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

M1 = 0x7FEB352D
M1_INVERSE = pow(M1, -1, 1 << 32)
U32 = np.uint32


def hash32(x):
    x = x ^ (x >> U32(16))
    x = x * U32(0x7FEB352D)
    x = x ^ (x >> U32(15))
    x = x * U32(0x846CA68B)
    return x ^ (x >> U32(16))


def frame_keys(seeds):
    """make_frame_keys: the two halves of the splitmix64 finaliser of every seed."""
    z = seeds.astype(np.uint64) + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    return (z & np.uint64(0xFFFFFFFF)).astype(U32), (z >> np.uint64(32)).astype(U32)


def inverse_of_odd(s):
    """s^-1 (mod 2^32) of odd words: Newton's iteration doubles the correct low bits (3 -> 6 -> 12 -> 24 -> 48)."""
    inv = s.copy()  # s * s = 1 (mod 8)
    for _ in range(4):
        inv = inv * (U32(2) - s * inv)
    return inv


def zero_word_positions(seeds, pixels):
    """position[i, j]: after how many steps the stream of pixel j under seed i draws the zero word ((sample << 12) + step)."""
    fa, fb = frame_keys(seeds)
    key = hash32(pixels[None, :] ^ fa[:, None])
    stride = hash32(key ^ fb[:, None]) | U32(1)
    y = (U32(0) - key) * U32(M1_INVERSE)
    counter = y ^ (y >> U32(16))
    return counter * inverse_of_odd(stride)


def kind_of(sample, step):
    scatter = step if sample == 0 else step - 1  # which scatter of the sample this step is (0: the jitter)
    return {0: "zero_jitter", 1: "redraw_first_scatter", 2: "redraw_second_scatter"}.get(scatter)


DIRECT_KINDS = ("zero_word_step_4", "zero_word_step_5")


def direct_kind_of(sample, step):
    """the kinds --direct adds: steps 4 and 5 of a sample > 0, named by their place in the stream"""
    return f"zero_word_step_{step}" if sample > 0 and step in (4, 5) else None


def search(width, height, max_sample, first_seed, seeds, block=1 << 16, max_step=3, kind_of=kind_of):
    pixels = np.arange(width * height, dtype=U32)
    found = []
    with np.errstate(over="ignore"):
        for start in range(first_seed, first_seed + seeds, block):
            block_seeds = np.arange(start, min(start + block, first_seed + seeds), dtype=np.uint64)
            position = zero_word_positions(block_seeds, pixels)
            sample, step = position >> U32(12), position & U32(4095)
            keep = (sample <= U32(max_sample)) & (step >= U32(1)) & (step <= U32(max_step))
            for i, j in zip(*np.nonzero(keep)):
                kind = kind_of(int(sample[i, j]), int(step[i, j]))
                if kind is not None:
                    found.append({"seed": int(block_seeds[i]), "width": width, "pixel": int(pixels[j]), "sample": int(sample[i, j]), "step": int(step[i, j]), "kind": kind})
    return found


def verified(entry):
    """The three draws of that step are 0.0, by the oracle's own stream."""
    from oracle import binding as oracle

    draws = oracle.random(entry["seed"], entry["pixel"], entry["sample"], 3 * entry["step"])
    return bool((draws[-3:].view(np.uint32) == 0).all())


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--width", type=int, default=8)
    ap.add_argument("--height", type=int, default=8)
    ap.add_argument("--max-sample", type=int, default=40, help="keep events at samples up to this one (frames of tens of samples)")
    ap.add_argument("--first-seed", type=int, default=0)
    ap.add_argument("--seeds", type=int, default=8_000_000)
    ap.add_argument("--per-kind", type=int, default=4, help="how many entries of each kind the fixture keeps (the lowest seeds)")
    ap.add_argument("--direct", action="store_true", help="keep steps 4 and 5 of a sample > 0 instead, for tests/golden/stream_events_direct.json")
    ap.add_argument("--out", default=None, help="default: tests/golden/stream_events.json, with --direct tests/golden/stream_events_direct.json")
    args = ap.parse_args()
    args.out = args.out or str(ROOT / "tests" / "golden" / ("stream_events_direct.json" if args.direct else "stream_events.json"))
    if args.direct:
        found = search(args.width, args.height, args.max_sample, args.first_seed, args.seeds, max_step=5, kind_of=direct_kind_of)
    else:
        found = search(args.width, args.height, args.max_sample, args.first_seed, args.seeds)
    kept = []
    for kind in DIRECT_KINDS if args.direct else ("redraw_first_scatter", "redraw_second_scatter", "zero_jitter"):
        of_kind = [e for e in found if e["kind"] == kind]
        print(f"{kind}: {len(of_kind)} found in {args.seeds} seeds x {args.width * args.height} pixels")
        kept += of_kind[: args.per_kind]
    for entry in kept:
        assert verified(entry), entry
    Path(args.out).write_text("[\n" + ",\n".join("  " + json.dumps(e) for e in kept) + "\n]\n")
    print(f"{len(kept)} entries -> {args.out}")


if __name__ == "__main__":
    main()
