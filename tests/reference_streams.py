"""What the unmodified reference wrote for coded bytes (tests/golden/streams_*.npz, made by
tests/golden/make_golden_streams.py), loaded once and handed out read-only.  A plain helper module of the suite, shared by
tests/test_reference_streams.py (CPU) and tests/test_gpu_reference_streams.py; it reads the fixtures only, never the
reference."""
import functools
import json
import os
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODES8 = [("qtable", "qtable", 0.0), ("none", "none", 0.0), ("divide40", "divide", 40.0), ("discard2", "discard", 2.0)]
# what the reference raises on a stream it cannot decode: int('', 2) and reshape are ValueErrors, a bad code its own type
REFUSALS = {"ValueError", "BadRleCodeError"}


@functools.lru_cache(maxsize=None)
def _load(name):
    with np.load(os.path.join(GOLDEN, name)) as z:
        out = {k: z[k] for k in z.files}
    for a in out.values():
        a.setflags(write=False)
    return out


def _json(a):
    return json.loads(bytes(a).decode())


# ---- (a), (e): step 8 alone -----------------------------------------------------------------------------------------------
def rle_index():
    return _json(_load("streams_rle.npz")["index"])


def streams():
    """[(name, N, zz int32 (nblocks, N*N), tuples, bytes, back)]"""
    z = _load("streams_rle.npz")
    out = []
    for s in rle_index()["streams"]:
        name = s["name"]
        tuples = [(0, 0) if (r == 0 and sz == 0) else (r, sz, a) for r, sz, a in z[name + "_rle"].tolist()]
        out.append((name, s["n"], z[name + "_zz"], tuples, z[name + "_bytes"].tobytes(), z[name + "_back"]))
    return out


def stream(name):
    return [s for s in streams() if s[0] == name][0]


def damaged():
    """[(name, N, nblocks, bytes, outcome, decoded array or None)]"""
    z = _load("streams_rle.npz")
    return [(d["name"], d["n"], d["nblocks"], z["dmg%d_bytes" % i].tobytes(), d["outcome"], z.get("dmg%d_back" % i))
            for i, d in enumerate(rle_index()["damaged"])]


# ---- (b): bands at dct_size 8 ---------------------------------------------------------------------------------------------
def band8_cases():
    return sorted({k.rsplit("_", 1)[0] for k in _load("streams_bands8.npz")})


def band8(case):
    """(input band, block size, {suffix: (mode, param, the reference's bytes, its decoded band)})"""
    c = _load("case_%s.npz" % case)
    z = _load("streams_bands8.npz")
    return c["input"], int(c["block_size"]), {s: (m, p, z["%s_%s" % (case, s)].tobytes(), c["band_" + s]) for s, m, p in MODES8}


# ---- (c): bands at other sizes --------------------------------------------------------------------------------------------
def band_n_cells():
    return _json(_load("streams_bands_n.npz")["cases"])


def band_n(i, band=None):
    """(cell, the reference's bytes, its decoded band or None).  `band`: the cell's input, to grow the tiles to its shape and
    to check that it is the band the reference was given."""
    z = _load("streams_bands_n.npz")
    cell = band_n_cells()[i]
    if band is not None:
        assert band.shape == (cell["h"], cell["w"])
        assert zlib.crc32(np.ascontiguousarray(band, dtype=np.int64).tobytes()) == cell["crc"], "not the band the reference coded"
    back = None
    if cell["decoded"]:
        bs = cell["bs"]
        back = np.repeat(np.repeat(z["b%d_tiles" % i], bs, axis=0), bs, axis=1)[:cell["h"], :cell["w"]]
    return cell, z["b%d_bytes" % i].tobytes(), back


# ---- (d): whole files -----------------------------------------------------------------------------------------------------
def file_configs():
    return _json(_load("streams_files.npz")["configs"])


def file_case(name, j=0):
    """(config record, RGB pixels, the reference's file or None, its decoded YCbCr pixels or None) of the configuration's
    picture j"""
    z = _load("streams_files.npz")
    rec = [c for c in file_configs() if c["name"] == name][0]
    data = z.get("%s_p%d_file" % (name, j))
    return rec, z[rec["rgb"][j]], None if data is None else data.tobytes(), z.get("%s_p%d_pixels" % (name, j))


def file_bands(name, j=0):
    """(the three 8-bit bands of picture j as Pillow converts them, the reference's three streams, its three decoded bands)"""
    from PIL import Image
    rec, rgb, blob, pixels = file_case(name, j)
    ycc = np.asarray(Image.fromarray(rgb, mode="RGB").convert("YCbCr"))
    head = int.from_bytes(blob[:2], "little")
    at, parts = head, []
    for _ in range(3):
        size = int.from_bytes(blob[at:at + 4], "little")
        parts.append(blob[at + 4:at + 4 + size])
        at += 4 + size
    assert at == len(blob)
    return [np.ascontiguousarray(ycc[:, :, c]) for c in range(3)], parts, [np.ascontiguousarray(pixels[:, :, c]) for c in range(3)]
