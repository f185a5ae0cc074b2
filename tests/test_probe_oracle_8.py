"""tests/probe_oracle_8.py held against the reference itself: tests/golden/probe8.npz holds len(Jpeg.compress), the coded bytes
of every band and the per-band squared error of Jpeg.decompress for two 37 x 53 pictures of streams_files.npz at dct_size 8,
block_size 1, 3 and 4 under divisors 1, 2, 3, 7, 40 and 1000 (tests/golden/make_golden_probe8.py).  CPU only."""
import ast
import json
import os

import numpy as np
import pytest
from PIL import Image

import probe_oracle_8 as po
from conftest import GOLDEN, REPO


@pytest.fixture(scope="module")
def fixture():
    z = np.load(os.path.join(GOLDEN, "probe8.npz"))
    index = json.loads(bytes(z["index"]))
    files = np.load(os.path.join(GOLDEN, "streams_files.npz"))
    pictures = [np.asarray(Image.fromarray(files[name], mode="RGB").convert("YCbCr")) for name in index["pictures"]]
    return z, index, pictures


def test_the_fixture_is_what_the_issue_asks_for(fixture):
    z, index, pictures = fixture
    assert index["block_sizes"] == [1, 3, 4] and index["divisors"] == [1, 2, 3, 7, 40, 1000]
    assert all(p.shape == (37, 53, 3) for p in pictures)
    # a container is its header, three length prefixes and three bands
    assert np.array_equal(z["file_len"], z["band_len"].sum(axis=2) + z["header_len"][:, None, :] + 12)
    assert os.path.getsize(os.path.join(GOLDEN, "probe8.npz")) < 16 * 1024


def test_sizes_are_the_reference(fixture):
    z, index, pictures = fixture
    params = [float(d) for d in index["divisors"]]
    for i, bs in enumerate(index["block_sizes"]):
        for p, pixels in enumerate(pictures):
            sizes, bad = po.band_sizes(po.picture_bands(pixels), bs, "divide", params)
            assert not bad.any()
            assert np.array_equal(sizes, z["band_len"][i, p]), (bs, p)


def test_squared_errors_are_the_reference(fixture):
    z, index, pictures = fixture
    params = [float(d) for d in index["divisors"]]
    for i, bs in enumerate(index["block_sizes"]):
        for p, pixels in enumerate(pictures):
            sse, bad = po.band_sse(po.picture_bands(pixels), bs, "divide", params)
            assert not bad.any()
            assert np.array_equal(sse, z["sse"][i, p]), (bs, p)


def test_moments_give_the_same_sum_as_the_pixels():
    """sum (v - s)^2 = S2 - 2 s S1 + cnt s^2 over the live pixels of a sample's tile: the identity the kernel relies on."""
    rng = np.random.default_rng(5)
    band = rng.integers(0, 256, (37, 53))
    for bs in (1, 3, 4):
        mom = po.band_moments(band, bs)
        h, w = mom.shape
        s = rng.integers(0, 256, (h, w))
        s1, s2 = (mom & np.uint64(0xFFFFFFFF)).astype(np.int64), (mom >> np.uint64(32)).astype(np.int64)
        live = np.zeros((h * bs, w * bs), np.int64)
        live[:37, :53] = 1
        cnt = live.reshape(h, bs, w, bs).sum(axis=(1, 3))
        back = np.repeat(np.repeat(s, bs, 0), bs, 1)[:37, :53]
        assert (s2 - 2 * s * s1 + cnt * s * s).sum() == ((band - back) ** 2).sum()


def test_the_helper_imports_nothing_of_the_product():
    tree = ast.parse(open(os.path.join(REPO, "tests", "probe_oracle_8.py")).read())
    imported = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            imported.update(a.name.split(".")[0] for a in node.names)
        elif isinstance(node, ast.ImportFrom):
            imported.add((node.module or "").split(".")[0] if node.level == 0 else "<relative>")
        elif isinstance(node, ast.Call) and getattr(node.func, "id", None) == "__import__":
            imported.add("<dynamic>")
    assert imported <= {"numpy", "oracle"}, imported
