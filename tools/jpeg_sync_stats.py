"""How fast a speculative Huffman decode of a baseline JPEG finds the true decoder state (CPU only).

The device decoder (csrc/jpeg_decode.hip) starts one lane per unit of `subseq_bits` bits from a guessed state
(bit position, block in MCU = 0, zig-zag index = 0).  This tool decodes one of the bench inputs
(tools/jpeg_bench.make_inputs: 640x480 q90 4:2:0) serially to get the true state at every symbol boundary, then
starts speculative decodes at random bits and records after how many bits the speculative state equals the true
one.  The share of starts that synchronise within S bits is the chance that a unit of S bits ends in the right state
after the speculative pass.

    python tools/jpeg_sync_stats.py --trials 300 --out profiles/r04_jpeg_sync_stats.txt
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from on_device_image_captioning_amd import jpeg as J  # noqa: E402


def destuffed_scan(blob, start):
    out, i = bytearray(), start
    while True:
        b = blob[i]
        if b != 0xFF:
            out.append(b)
            i += 1
        elif blob[i + 1] == 0:
            out.append(0xFF)
            i += 2
        else:
            return bytes(out)                              # EOI (the inputs carry no restart markers)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=300)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--image", type=int, default=1, help="index into jpeg_bench.make_inputs")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import jpeg_bench
    blob = jpeg_bench.make_inputs(args.image + 1)[args.image]
    hd = J.parse(blob)
    assert hd.kind == J.DEVICE and hd.restart_interval == 0
    tabs = [J.device_tables(t) for t in hd.dc_tables + hd.ac_tables]
    seg = destuffed_scan(blob, hd.data_offset)
    bits = int.from_bytes(seg + b"\xff" * 8, "big")
    nbits, end = (len(seg) + 8) * 8, len(seg) * 8
    nY = (1, 2, 4)[hd.sampling]
    bpm = nY + 2

    def lookup(t, peek16):
        lut, maxcode, valoff, huffval = tabs[t]
        e = int(lut[peek16 >> (16 - J.LUT_BITS)])
        if e:
            return e >> 8, e & 255
        for length in range(J.LUT_BITS + 1, 17):
            code = peek16 >> (16 - length)
            if code <= maxcode[length]:
                return length, int(huffval[code + valoff[length]])
        return None

    def step(pos, blk, k):                                 # the device's `step`, without the coefficient value
        c = 0 if blk < nY else blk - nY + 1
        r = lookup(c if k == 0 else 3 + c, (bits >> (nbits - pos - 16)) & 0xFFFF)
        if r is None:
            return None
        ln, sym = r
        if k == 0:
            return pos + ln + sym, blk, 1
        run, size = sym >> 4, sym & 15
        if size:
            k, pos = k + run + 1, pos + ln + size
        else:
            pos, k = pos + ln, (k + 16 if run == 15 else 64)
        if k >= 64:
            k, blk = 0, (blk + 1) % bpm
        return pos, blk, k

    true = {}
    st = (0, 0, 0)
    while st[0] < end:
        true[st[0]] = st[1:]
        st = step(*st)
    rng = np.random.default_rng(args.seed)
    dist = []
    for _ in range(args.trials):
        x = int(rng.integers(0, end - 20000))
        st = (x, 0, 0)
        while st is not None and st[0] < end and not (st[0] in true and true[st[0]] == st[1:]):
            st = step(*st)
        dist.append(st[0] - x if st is not None and st[0] < end else -1)
    d = np.array(dist)
    lines = [f"image: jpeg_bench.make_inputs[{args.image}], {len(blob)} bytes, {end} scan bits, {len(true)} symbols",
             f"speculative starts: {args.trials} random bits, guess (block 0, zig-zag 0), seed {args.seed}"]
    for S in (512, 1024, 2048, 4096, 8192, 20000):
        lines.append(f"synchronised within {S:5d} bits: {100 * np.mean((d >= 0) & (d < S)):5.1f} %")
    lines.append(f"never synchronised before the end of the scan: {100 * np.mean(d < 0):.1f} %")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
