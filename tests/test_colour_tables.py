"""The integer tables of Pillow's RGB <-> YCbCr conversion (tests/golden/colour_tables.npz, recovered from Pillow by
tests/golden/make_colour_tables.py): the NumPy model over them (tests/colour_model.py) equals the installed Pillow on every
colour in both directions, and the include the kernels are built from holds the same integers.  CPU only."""
import os
import re

import numpy as np
import pytest

import colour_model
from conftest import REPO


@pytest.fixture(scope="module")
def every():
    a = colour_model.all_colours()
    a.setflags(write=False)
    return a


def test_the_picture_holds_every_colour_once(every):
    flat = every.reshape(-1, 3).astype(np.uint32)
    assert np.array_equal((flat[:, 0] << 16) | (flat[:, 1] << 8) | flat[:, 2], np.arange(1 << 24, dtype=np.uint32))


@pytest.mark.parametrize("src, dst, model", [("RGB", "YCbCr", colour_model.rgb_to_ycbcr), ("YCbCr", "RGB", colour_model.ycbcr_to_rgb)])
def test_model_equals_pillow_on_every_colour(every, src, dst, model):
    from PIL import Image
    want = np.asarray(Image.fromarray(every, mode=src).convert(dst))
    got = model(every)
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert int(np.count_nonzero(got != want)) == 0


def test_the_include_holds_the_tables_of_the_npz():
    text = open(os.path.join(REPO, "include", "jpegx_colour_tables.inc")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    tables = colour_model.load_tables()
    names = colour_model.FORWARD_TABLES + colour_model.INVERSE_TABLES
    found = re.findall(r"#define\s+JPEGX_COLOUR_([A-Z_]+)\s*\\\n((?:[ \t]*[-0-9, ]+\\?\n)+)", text)
    assert [n for n, _ in found] == [n.upper() for n in names]
    for name, body in found:
        values = np.array([int(v) for v in re.findall(r"-?\d+", body)])
        assert values.shape == (256,), name
        assert np.array_equal(values, tables[name.lower()]), name
        assert np.abs(values).max() <= 32767, name          # int16 initialisers
    with np.load(colour_model.TABLES_PATH) as raw:
        assert sorted(raw.files) == sorted(names)
        assert all(raw[k].dtype == np.int16 and raw[k].shape == (256,) for k in raw.files)
