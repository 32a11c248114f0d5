"""The reference's dat/default_camb_Cls.jld2, rebuilt byte for byte from tests/golden/default_camb_Cls_jld2_parts.npz and
tests/golden/camb_cls.npz (tools/make_jld2_fixture.py stored it that way: the file itself is 2 MB)."""
import hashlib
import lzma
import os
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def write_reference_jld2(path):
    p = np.load(os.path.join(GOLDEN, "default_camb_Cls_jld2_parts.npz"))
    z = np.load(os.path.join(GOLDEN, "camb_cls.npz"))
    skel = lzma.decompress(p["skeleton_xz"].tobytes())
    ns, nb = (int(x) for x in p["tail_shape"])
    tail = np.frombuffer(lzma.decompress(p["tail_xz"].tobytes()), np.uint8)
    tail = np.ascontiguousarray(tail.reshape(ns, 8, nb).transpose(0, 2, 1)).view("<f8").reshape(ns, nb)
    out, pos = bytearray(), 0                     # pos: read position in the skeleton
    for off, key, t in zip(p["offsets"], p["prefix_keys"], tail):
        take = int(off) - len(out)                # metadata between the previous stream and this one
        out += skel[pos:pos + take]
        pos += take
        out += zlib.compress(np.concatenate([z[str(key)], t]).astype("<f8").tobytes(), 6)
    out += skel[pos:]
    digest = hashlib.sha256(out).hexdigest()
    assert digest == str(p["sha256"]), "rebuilt file differs from the reference's (is Python's zlib a different deflate implementation?)"
    with open(path, "wb") as fh:
        fh.write(out)
    return path
