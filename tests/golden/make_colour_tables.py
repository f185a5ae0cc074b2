#!/usr/bin/env python3
"""The installed Pillow's RGB <-> YCbCr conversion -> tests/golden/colour_tables.npz -> include/jpegx_colour_tables.inc.

Pillow converts in fixed point (scale 2^6) through per-channel tables; tests/colour_model.py states the formulas.  The
luma tables are floor(c * 64 * i + 0.5); the chroma tables are no rounding of the textbook coefficients, so they are
RECOVERED here from what Pillow gives for every colour:

  * d_r[Cr] and d_b[Cb] are read as out - Y wherever the result lies strictly inside 0..255 (one value per index, the
    same at every such Y);
  * the pairs (cb_r, cb_g), (cr_g, cr_b), (g_cb, g_cr) satisfy  64 o <= T1[u] + T2[v] + 32 w <= 64 o + 63  for every
    output o (its +128 taken off): difference constraints in T1 and -T2, solved by Bellman-Ford sweeps over the
    256 x 256 grid.  A solution is not unique; any that reproduces Pillow is right.

Nothing is written unless the model with the recovered tables equals Pillow on all 2^24 inputs in both directions.
"""
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
import colour_model  # noqa: E402

I = np.arange(256)


def convert(pixels, src, dst):
    return np.asarray(Image.fromarray(pixels, src).convert(dst))


def solve(lo, hi, t2_guess):
    """Integers T1[256], T2[256] with lo[u][v] <= T1[u] + T2[v] <= hi[u][v], or None.  With z = -T2 the constraints are
    T1[u] - z[v] <= hi and z[v] - T1[u] <= -lo: shortest-path relaxations from the guess until nothing moves."""
    lo, hi = lo.astype(np.int64), hi.astype(np.int64)
    z = -t2_guess.astype(np.int64)
    t1 = np.min(hi + z[None, :], axis=1)
    for _ in range(2000):
        nt1 = np.minimum(t1, np.min(hi + z[None, :], axis=1))
        nz = np.minimum(z, np.min(nt1[:, None] - lo, axis=0))
        if np.array_equal(nt1, t1) and np.array_equal(nz, z):
            break
        t1, z = nt1, nz
    s = t1[:, None] - z[None, :]
    return (t1, -z) if bool(np.all((s >= lo) & (s <= hi))) else None


def one_value_per_index(delta, valid, axis_kept):
    """delta where valid, reduced over every axis but ``axis_kept``: the single value each index shows, else None."""
    other = tuple(a for a in range(delta.ndim) if a != axis_kept)
    top = np.where(valid, delta, -(1 << 20)).max(axis=other)
    low = np.where(valid, delta, 1 << 20).min(axis=other)
    return top if np.array_equal(top, low) else None


def recover():
    every = colour_model.all_colours()
    t = {}
    # ---- forward: cube[r][g][b] ------------------------------------------------------------------------------------
    ycc = convert(every, "RGB", "YCbCr").reshape(256, 256, 256, 3)
    for name, c in (("y_r", 0.299), ("y_g", 0.587), ("y_b", 0.114)):
        t[name] = np.floor(c * 64 * I + 0.5).astype(np.int64)
    w = 32 * I.astype(np.int32)
    o = ycc[..., 1].astype(np.int32) - 128                               # Cb - 128 = (cb_r[r] + cb_g[g] + 32 b) >> 6
    pair = solve((64 * o - w[None, None, :]).max(axis=2), (64 * o + 63 - w[None, None, :]).min(axis=2),
                 np.trunc(-0.331264 * 64 * I))
    if pair is None:
        raise SystemExit("no tables reproduce Pillow's Cb")
    t["cb_r"], t["cb_g"] = pair
    o = ycc[..., 2].astype(np.int32) - 128                               # Cr - 128 = (32 r + cr_g[g] + cr_b[b]) >> 6
    pair = solve((64 * o - w[:, None, None]).max(axis=0), (64 * o + 63 - w[:, None, None]).min(axis=0),
                 np.trunc(-0.081312 * 64 * I))
    if pair is None:
        raise SystemExit("no tables reproduce Pillow's Cr")
    t["cr_g"], t["cr_b"] = pair
    # ---- inverse: cube[y][cb][cr] ----------------------------------------------------------------------------------
    rgb = convert(every, "YCbCr", "RGB").reshape(256, 256, 256, 3).astype(np.int32)
    delta = rgb - I.astype(np.int32)[:, None, None, None]
    inside = (rgb > 0) & (rgb < 255)
    t["d_r"] = one_value_per_index(delta[..., 0], inside[..., 0], 2)
    t["d_b"] = one_value_per_index(delta[..., 2], inside[..., 2], 1)
    if t["d_r"] is None or t["d_b"] is None:
        raise SystemExit("Pillow's R or B is no Y + table[chroma]")
    top = np.where(inside[..., 1], delta[..., 1], -(1 << 20)).max(axis=0)
    low = np.where(inside[..., 1], delta[..., 1], 1 << 20).min(axis=0)
    if not np.array_equal(top, low):
        raise SystemExit("Pillow's G is no Y + f(Cb, Cr)")
    pair = solve(64 * top, 64 * top + 63, np.trunc(-0.714136 * 64 * (I - 128)))
    if pair is None:
        raise SystemExit("no tables reproduce Pillow's G")
    t["g_cb"], t["g_cr"] = pair
    # ---- the criterion: every colour, both directions --------------------------------------------------------------
    for k, v in t.items():
        if np.abs(v).max() > 32767:
            raise SystemExit("table %s does not fit int16" % k)
    t = {k: v.astype(np.int32) for k, v in t.items()}
    bad_f = int(np.count_nonzero(colour_model.rgb_to_ycbcr(every, t) != ycc.reshape(every.shape)))
    bad_i = int(np.count_nonzero(colour_model.ycbcr_to_rgb(every, t) != rgb.reshape(every.shape)))
    if bad_f or bad_i:
        raise SystemExit("the recovered tables miss Pillow: %d bytes forward, %d inverse -- nothing written" % (bad_f, bad_i))
    return {k: v.astype(np.int16) for k, v in t.items()}


def intarr(a, per=16):
    flat = np.asarray(a).ravel()
    return " \\\n".join("    " + ", ".join(str(int(v)) for v in flat[k:k + per]) + "," for k in range(0, flat.size, per))


def write_inc(npz_path, inc_path):
    t = np.load(npz_path)
    what = {"y_r": "Y from R: floor(0.299 * 64 * i + 0.5)", "y_g": "Y from G: floor(0.587 * 64 * i + 0.5)",
            "y_b": "Y from B: floor(0.114 * 64 * i + 0.5)", "cb_r": "Cb from R", "cb_g": "Cb from G (B enters as 32 * b)",
            "cr_g": "Cr from G (R enters as 32 * r)", "cr_b": "Cr from B", "d_r": "R - Y by Cr", "g_cb": "G from Cb, scale 2^6",
            "g_cr": "G from Cr, scale 2^6", "d_b": "B - Y by Cb"}
    parts = [
        "/* GENERATED by tests/golden/make_colour_tables.py from tests/golden/colour_tables.npz.\n"
        " * DATA ONLY: the integer tables of Pillow's RGB <-> YCbCr conversion (Image.convert), recovered from Pillow's\n"
        " * outputs and checked against it on all 2^24 inputs in both directions (formulas: tests/colour_model.py);\n"
        " * int16 initialisers, 256 entries each; do not edit by hand. */",
        "#ifndef JPEGX_COLOUR_TABLES_INC\n#define JPEGX_COLOUR_TABLES_INC",
    ]
    for name in colour_model.FORWARD_TABLES + colour_model.INVERSE_TABLES:
        parts.append("/* %s */\n#define JPEGX_COLOUR_%s \\\n%s" % (what[name], name.upper(), intarr(t[name])))
    parts.append("#endif")
    with open(inc_path, "w") as f:
        f.write("\n\n".join(parts) + "\n")


def main():
    npz_path = os.path.join(HERE, "colour_tables.npz")
    np.savez(npz_path, **recover())
    write_inc(npz_path, os.path.join(REPO, "include", "jpegx_colour_tables.inc"))
    print("written: %s and include/jpegx_colour_tables.inc (Pillow %s)" % (os.path.relpath(npz_path, REPO), Image.__version__))


if __name__ == "__main__":
    main()
