#!/usr/bin/env python3
"""Store the reference's dat/default_camb_Cls.jld2 (2 MB, written by the JLD2 package) in a form small enough for the repository:
    python tools/make_jld2_fixture.py <path to the reference's dat/default_camb_Cls.jld2>
-> tests/golden/default_camb_Cls_jld2_parts.npz.  The file is 26 kB of JLD2 metadata plus 21 zlib streams, one Float64 vector of
15998 values per spectrum (tools/extract_cls.py).  The first 11999 values of every vector are already in tests/golden/camb_cls.npz;
kept here are the metadata with the streams cut out, where each stream sat, which camb_cls.npz array it starts with, the values
beyond (byte-shuffled, xz) and the file's SHA-256.  tests/_ref_jld2.py rebuilds the file byte for byte: the streams are zlib
level 6, which this script checks."""
import hashlib
import lzma
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DST = os.path.join(ROOT, "tests", "golden", "default_camb_Cls_jld2_parts.npz")
NL, LEVEL = 15998, 6


def streams(buf):
    """(offset, length, vector) of every zlib stream that inflates to one NL-element Float64 vector, in file order"""
    out, i = [], 0
    while True:
        j = buf.find(b"\x78\x9c", i)
        if j < 0:
            return out
        d = zlib.decompressobj()
        try:
            raw = d.decompress(buf[j:])
        except zlib.error:
            raw = b""
        if d.eof and len(raw) == 8 * NL:
            n = len(buf) - j - len(d.unused_data)
            out.append((j, n, np.frombuffer(raw, "<f8")))
            i = j + n
        else:
            i = j + 1


def main(src):
    buf = open(src, "rb").read()
    z = np.load(os.path.join(ROOT, "tests", "golden", "camb_cls.npz"))
    n = len(z["ell"])
    st = streams(buf)
    assert len(st) == 21, len(st)
    skel, keys, pos = [], [], 0
    for off, ln, v in st:
        assert zlib.compress(v.tobytes(), LEVEL) == buf[off:off + ln], "stream is not zlib level 6"
        keys.append(next(k for k in z.files if k != "ell" and np.array_equal(z[k], v[:n])))
        skel.append(buf[pos:off])
        pos = off + ln
    skel.append(buf[pos:])
    tail = np.stack([v[n:] for _, _, v in st])
    shuffled = np.ascontiguousarray(tail.view(np.uint8).reshape(len(st), -1, 8).transpose(0, 2, 1))
    np.savez(DST, skeleton_xz=np.frombuffer(lzma.compress(b"".join(skel), preset=9), np.uint8),
             offsets=np.array([off for off, _, _ in st]), prefix_keys=np.array(keys), tail_shape=np.array(tail.shape),
             tail_xz=np.frombuffer(lzma.compress(shuffled.tobytes(), preset=9 | lzma.PRESET_EXTREME), np.uint8),
             sha256=np.array(hashlib.sha256(buf).hexdigest()))
    print(DST, os.path.getsize(DST), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
