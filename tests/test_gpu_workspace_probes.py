"""GPU: the size probes and the distortion probes from pixels -- stacks of pictures at dct_size 8 (jpegx_batch_probe_pictures,
jpegx_batch_probe_distortion_pictures), at any other size (the _n entries) and sets of unequal sizes
(jpegx_batch_probe_picture_set_n, jpegx_batch_probe_distortion_picture_set_n) -- each in a workspace of exactly the size its
jpegx_batch_probe*_workspace_bytes* function declares, 16-byte aligned and no more, between two guards
(tests/workspace_fence.py).  The workspace is one group of float64 planes (and as much again for the moments), rounded up to
256 bytes, so the cases aim at the group: a lone picture, three groups of one, a short last group, a 1 x 1 picture in a set.

The yardsticks are product-free: tests/probe_oracle_8.py at 8 x 8; elsewhere, candidate by candidate, the length of
tests/codec_oracle_n.py's stream and the squared error of its decoded band, on content it finds free of rounding ties.
K = 1 and K = JPEGX_PROBE_MAX_CANDIDATES = 32 in every quantiser mode an entry takes; every mode and K of a case runs on ONE
workspace that is never refilled, so each call but the first starts from what the last one left."""
import numpy as np
import pytest

import probe_oracle_8 as p8
import workspace_roads as wr
from fenced import Fenced
from workspace_fence import FencedWorkspace, fences

pytestmark = pytest.mark.gpu

BAD = np.uint64(1 << 63)
K_MAX = 32
# 4 x odd: a forward tie d (m + 1/2) is then 2 x odd, which no multiple of 16 is (samples that are multiples of 64, matrix
# products with denominators up to 4), and the N = 2 inverse, a sum of restored coefficients over 4, stays an integer
DIVISORS = [4.0 * (2 * q + 7) for q in range(K_MAX)]
KEEPS = [float(q) for q in range(K_MAX)]


def candidates(eight):
    """(mode, params) in every mode the entries take, K = 1 and K = 32."""
    out = [("none", [0.0]), ("discard", KEEPS[2:3]), ("discard", KEEPS), ("divide", DIVISORS[3:4]), ("divide", DIVISORS)]
    return out + [("qtable", [0.0])] if eight else out


def run_probe(gpu, entry, args, nplanes, mode, params, ws, tail):
    """One probe call on the fenced workspace -> (low bits int64 [nplanes][K], bad bool [nplanes][K])."""
    dtot = Fenced(gpu, nplanes * len(params) * 8)
    try:
        entry(*args, mode, params, *tail(ws.ptr, dtot.ptr))
        raw = dtot.download(what="the totals").view(np.uint64).reshape(nplanes, len(params))
    finally:
        dtot.free()
    return (raw & ~BAD).astype(np.int64), (raw & BAD) != 0


def check(got, want, what):
    (low, bad), (want_low, want_bad) = got, want
    assert np.array_equal(bad, want_bad), what
    assert np.array_equal(low[~bad], np.asarray(want_low)[~bad]), what


# ---- dct_size 8 -----------------------------------------------------------------------------------------------------------------
# (pictures, bands, rows, cols, block_size, colour, group_planes): what the case aims at
CASES_8 = {
    "lone": ((1, 1, 7, 5, 1, 0, 1), "a lone picture of one block: the smallest group"),
    "three-groups-rgb": ((3, 3, 10, 11, 3, 1, 3), "RGB, ragged at block_size 3, three groups of one picture"),
    "short-last": ((5, 1, 9, 17, 1, 0, 2), "five pictures in groups of two: the last group is shorter"),
    "one-group-bs2": ((2, 4, 30, 33, 2, 0, 8), "four bands at block_size 2, both pictures in one group"),
}


@fences("jpegx_batch_probe_pictures_workspace_bytes", "jpegx_batch_probe_distortion_pictures_workspace_bytes")
@pytest.mark.parametrize("name", list(CASES_8))
def test_probes_at_dct_size_8(gpu, name):
    (k, nb, rows, cols, bs, colour, gp), aim = CASES_8[name]
    pixels = wr.noise_pictures(3, [(rows, cols)] * k, nb)
    bands = [b for px in pixels for b in p8.picture_bands(wr.model_of(px, colour))]
    shape = (k, nb, rows, cols, bs)
    din = Fenced(gpu, k * rows * cols * nb)
    ws_s = FencedWorkspace(gpu, gpu.batch_probe_pictures_workspace_bytes(*shape, gp), 16)
    ws_d = FencedWorkspace(gpu, gpu.batch_probe_distortion_pictures_workspace_bytes(*shape, gp), 16)
    assert ws_d.nbytes == 2 * ws_s.nbytes
    try:
        din.upload(np.concatenate([p.reshape(-1) for p in pixels]))
        for mode, params in candidates(True):
            what = "%s (%s) %s K %d" % (name, aim, mode, len(params))
            tail = lambda w, t: (gp, w, t, colour)
            check(run_probe(gpu, gpu.batch_probe_pictures_device, (din.ptr, *shape), k * nb, mode, params, ws_s, tail),
                  p8.band_sizes(bands, bs, mode, params), what + " sizes")
            ws_s.check(what + " sizes")
            check(run_probe(gpu, gpu.batch_probe_distortion_pictures_device, (din.ptr, *shape), k * nb, mode, params, ws_d, tail),
                  p8.band_sse(bands, bs, mode, params), what + " distortion")
            ws_d.check(what + " distortion")
        din.download(what="the pixels")
    finally:
        din.free()
        ws_s.free()
        ws_d.free()


# ---- any other dct_size ---------------------------------------------------------------------------------------------------------
def yardstick(kind, pictures, bs, n, mode, params, colour, group):
    """(sizes, squared errors) int64 [nplanes][K] from the codec oracle run once per candidate; wr.TieError on a tie."""
    nb = pictures[0].shape[2]
    models = [wr.model_of(p, colour)[:, :, b].astype(np.int64) for p in pictures for b in range(nb)]
    sizes, sse = [], []
    for q in params:
        road = wr.Road(kind, pictures, bs, n, mode, q, colour=colour, group=group)
        sizes.append([len(b) for b in road.blobs])
        sse.append([int(((m - np.asarray(d, np.int64)) ** 2).sum()) for m, d in zip(models, road.decoded_bands)])
    return np.array(sizes, np.int64).T, np.array(sse, np.int64).T


def content(kind, sizes, nb, bs, n, colour, group):
    """[(mode, params, pictures, yardstick)] in every mode, each free of ties under every candidate.  Two sets of pictures: under
    'divide' multiples of 64 (codec_oracle_n.make_band's step under a divisor of 40) up to the peak that 40 still codes; under
    'none' and 'discard' multiples of 4 up to the peak whose DC, N^2 times the sample, codes in 15 bits -- 15 at N = 32."""
    def make(seed):
        out = []
        for content_mode, content_param in (("none", 0.0), ("divide", 40.0)):
            px = wr.free_pictures(seed, sizes, nb, bs, n, content_mode, content_param, grey=bool(colour))
            out += [(mode, params, px, yardstick(kind, px, bs, n, mode, params, colour, group)) for mode, params in candidates(False)
                    if (mode == "divide") == (content_mode == "divide")]
        return out
    return wr.build(make)


# n, (pictures, bands, rows, cols, block_size, colour, group_planes)
CASES_N = {
    "N2-three-groups": (2, (3, 3, 10, 11, 3, 0, 3), "N 2, ragged at block_size 3, three groups of one picture"),
    "N3-lone-rgb": (3, (1, 3, 7, 11, 1, 1, 3), "N 3: a lone RGB picture"),
    "N32-short-last": (32, (5, 1, 33, 20, 1, 0, 2), "N 32: five pictures of two blocks in groups of two, the last shorter"),
}


@fences("jpegx_batch_probe_pictures_workspace_bytes_n", "jpegx_batch_probe_distortion_pictures_workspace_bytes_n")
@pytest.mark.parametrize("name", list(CASES_N))
def test_probes_at_any_other_dct_size(gpu, name):
    n, (k, nb, rows, cols, bs, colour, gp), aim = CASES_N[name]
    wanted = content("pictures", [(rows, cols)] * k, nb, bs, n, colour, gp)
    shape = (k, nb, rows, cols, bs, n)
    din = Fenced(gpu, k * rows * cols * nb)
    ws_s = FencedWorkspace(gpu, gpu.batch_probe_pictures_workspace_bytes_n(*shape, gp), 16)
    ws_d = FencedWorkspace(gpu, gpu.batch_probe_distortion_pictures_workspace_bytes_n(*shape, gp), 16)
    assert ws_d.nbytes == 2 * ws_s.nbytes
    try:
        for mode, params, pixels, (sizes, sse) in wanted:
            din.upload(np.concatenate([p.reshape(-1) for p in pixels]))
            what = "%s (%s) %s K %d" % (name, aim, mode, len(params))
            tail = lambda w, t: (gp, w, t, colour)
            clean = np.zeros(sizes.shape, bool)
            check(run_probe(gpu, gpu.batch_probe_pictures_n_device, (din.ptr, *shape), k * nb, mode, params, ws_s, tail), (sizes, clean), what + " sizes")
            ws_s.check(what + " sizes")
            check(run_probe(gpu, gpu.batch_probe_distortion_pictures_n_device, (din.ptr, *shape), k * nb, mode, params, ws_d, tail), (sse, clean),
                  what + " distortion")
            ws_d.check(what + " distortion")
        din.download(what="the pixels")
    finally:
        din.free()
        ws_s.free()
        ws_d.free()


# n, sizes, bands, block_size, colour, group_samples
SET_CASES = {
    "N2-three-groups-rgb": (2, [(9, 14), (1, 1), (5, 23)], 3, 1, 1, 4, "RGB, every picture a group of its own, a 1 x 1 picture among them"),
    "N3-short-last": (3, [(5, 7), (6, 6), (1, 1), (3, 2), (11, 5)], 1, 2, 0, 27, "block_size 2, groups of at most 27 samples, the last shorter"),
    "N32-one-group": (32, [(33, 20), (1, 1), (30, 40)], 1, 1, 0, 0, "N 32, one group of 2 + 1 + 2 blocks"),
}


@fences("jpegx_batch_probe_picture_set_workspace_bytes_n", "jpegx_batch_probe_distortion_picture_set_workspace_bytes_n")
@pytest.mark.parametrize("name", list(SET_CASES))
def test_probes_of_sets(gpu, name):
    n, sizes, nb, bs, colour, gs, aim = SET_CASES[name]
    wanted = content("set", sizes, nb, bs, n, colour, gs)
    table = gpu.picture_set_table(sizes, nb, bs, n)
    nplanes = len(sizes) * nb
    din, dtab = Fenced(gpu, sum(r * c * nb for r, c in sizes)), gpu.DeviceBuffer(table.blob.nbytes)
    ws_s = FencedWorkspace(gpu, gpu.batch_probe_picture_set_workspace_bytes_n(table, gs), 16)
    ws_d = FencedWorkspace(gpu, gpu.batch_probe_distortion_picture_set_workspace_bytes_n(table, gs), 16)
    assert ws_d.nbytes == 2 * ws_s.nbytes
    try:
        dtab.upload(table.blob)
        for mode, params, pixels, (want_sizes, sse) in wanted:
            din.upload(np.concatenate([p.reshape(-1) for p in pixels]))
            what = "%s (%s) %s K %d" % (name, aim, mode, len(params))
            tail = lambda w, t: (w, t, colour, gs)
            clean = np.zeros(want_sizes.shape, bool)
            check(run_probe(gpu, gpu.batch_probe_picture_set_n_device, (din.ptr, table, dtab.ptr), nplanes, mode, params, ws_s, tail), (want_sizes, clean),
                  what + " sizes")
            ws_s.check(what + " sizes")
            check(run_probe(gpu, gpu.batch_probe_distortion_picture_set_n_device, (din.ptr, table, dtab.ptr), nplanes, mode, params, ws_d, tail),
                  (sse, clean), what + " distortion")
            ws_d.check(what + " distortion")
        din.download(what="the pixels")
    finally:
        din.free()
        dtab.free()
        ws_s.free()
        ws_d.free()


def contents():
    """(id, the content of a case): what tests/test_workspace_sizes.py builds on the CPU."""
    for name, (n, (k, nb, rows, cols, bs, colour, gp), _) in CASES_N.items():
        yield name, content("pictures", [(rows, cols)] * k, nb, bs, n, colour, gp)
    for name, (n, sizes, nb, bs, colour, gs, _) in SET_CASES.items():
        yield "set-" + name, content("set", sizes, nb, bs, n, colour, gs)
