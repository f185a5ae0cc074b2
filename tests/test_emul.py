"""Host build of the kernels' arithmetic (csrc/jpegx_math.h via tests/emul/emul.cpp) against the
oracle: the fp32 fast tier + error bound + float64 exact tier must reproduce the reference's
integers bit for bit, and the observed fp32 error must sit far inside the bound.  CPU only."""
import ctypes

import numpy as np
import pytest

import emul_lib
import oracle
from conftest import CASES, MODES


@pytest.fixture(scope="module")
def emul():
    return emul_lib.load()


def _p(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t))


AAN_G = np.array([1, 1.9615705608064609, 1.8477590650225733, 1.6629392246050902, 1.4142135623730947, 1.1111404660392048,
                  0.76536686473017901, 0.3901806440322565])       # JPEGX_AAN_G (csrc/jpegx_math.h, tests/derive_bounds.py)


def rq_table(mode, param):
    """The fp32 multipliers the fused kernels get: the quantiser's reciprocal with the scale of the AAN transform's
    output folded in, formed in double and rounded once (jpegx_internal.h scale_for_aan)."""
    qt = oracle.tables()["qtable"].ravel().astype(np.float64)
    if mode == "qtable":
        r = 1.0 / qt
    elif mode == "none":
        r = np.ones(64)
    elif mode == "divide":
        r = np.full(64, 1.0 / param)
    else:
        r = np.zeros((8, 8))
        r[:int(param), :int(param)] = 1
        r = r.ravel()
    return (r / np.outer(AAN_G, AAN_G).ravel()).astype(np.float32)


def run_forward(lib, plane, mode, param, pixel):
    a = np.ascontiguousarray(plane, np.float32)
    h, w = a.shape
    rq = rq_table(mode, param)
    out = np.empty((h // 8, w // 8, 64), np.int16)
    st = np.zeros(4)
    dc_exact = int(bool(pixel) and np.frexp(rq[0])[0] == 0.5 and (mode != "divide" or float(rq[0]) * param == 1.0))
    lib.emul_forward(_p(a, ctypes.c_float), h, w, oracle.MODE_BY_NAME[mode], ctypes.c_double(param),
                     _p(rq, ctypes.c_float), int(pixel), dc_exact, _p(out, ctypes.c_int16), None,
                     _p(st, ctypes.c_double))
    return out, st


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("suffix,mode,param", MODES)
def test_forward_two_tier_matches_reference(emul, golden, case, suffix, mode, param):
    c = golden(case)
    for pixel in (1, 0):
        got, st = run_forward(emul, c["pre"], mode, param, pixel)
        assert np.array_equal(got, c["zz_" + suffix])
        assert st[2] < 1.0           # observed |t32 - t64| vs the per-coefficient bound F(k, l) u S / q


@pytest.mark.parametrize("kind", ["noise", "smooth"])
def test_forward_two_tier_large(emul, kind):
    from jpegx import synth
    a = synth.generate_plane(kind, 512, 512, seed=9)
    for mode, param in (("qtable", 0.0), ("divide", 7.0), ("none", 0.0)):
        got, st = run_forward(emul, a, mode, param, 1)
        assert np.array_equal(got, oracle.forward_f32(a, mode, param))
        # typical error sits well inside the bound; the worst case on these planes is the DC coefficient under
        # `divide 7`: it is computed exactly, the bound charges one rounding (that of the fp32 reciprocal) and
        # fl32(1/7) happens to be off by 0.75 u
        assert st[2] < 0.8
    _, st = run_forward(emul, a, "qtable", 0.0, 1)
    assert st[1] / (a.size / 64) < 0.08   # exact-tier share of blocks stays small for the JPEG table


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("suffix,mode,param", MODES)
def test_inverse_two_tier_matches_reference(emul, golden, case, suffix, mode, param):
    c = golden(case)
    zz = np.ascontiguousarray(c["zz_" + suffix])
    h, w = zz.shape[0] * 8, zz.shape[1] * 8
    out = np.empty((h, w), np.int32)
    st = np.zeros(4)
    emul.emul_inverse(_p(zz, ctypes.c_int16), h, w, oracle.MODE_BY_NAME[mode], ctypes.c_double(param),
                      _p(out, ctypes.c_int32), _p(st, ctypes.c_double))
    assert np.array_equal(out, c["idct_" + suffix])
    assert st[2] < 1.0               # observed fp32 error / bound u (3/32 |DC| + 9/32 A1 + 3/4 A2), jpegx_math.h


def run_inverse(lib, zz, mode, param):
    zz = np.ascontiguousarray(zz, np.int16)
    h, w = zz.shape[0] * 8, zz.shape[1] * 8
    out = np.empty((h, w), np.int32)
    st = np.zeros(4)
    lib.emul_inverse(_p(zz, ctypes.c_int16), h, w, oracle.MODE_BY_NAME[mode], ctypes.c_double(param),
                     _p(out, ctypes.c_int32), _p(st, ctypes.c_double))
    return out, st


def test_inverse_bound_holds_on_adversarial_blocks(emul):
    """The a-priori bound of the inverse fast tier is an L1 bound: it is approached when every coefficient
    pushes one output sample in the same direction.  Blocks whose signs follow sign(C[k][i] C[l][j]) for
    every target sample (i, j), at several magnitudes and sparsity patterns, plus random sign patterns:
    the observed fp32 error never reaches the bound and the two-tier result equals the oracle's."""
    t = oracle.tables()
    C = t["dct_matrix"]
    zigzag = t["zigzag8"]
    rng = np.random.default_rng(77)
    blocks = []
    for i in range(8):
        for j in range(8):
            sign = np.sign(np.outer(C[:, i], C[:, j]))
            for mag in (1, 37, 1000, 16383):
                blocks.append(sign * mag)
                blocks.append(sign * rng.integers(0, mag + 1, (8, 8)))
            only_inner = sign * 900
            only_inner[0, :] = 0
            only_inner[:, 0] = 0
            blocks.append(only_inner)
            first_rc = np.zeros((8, 8))
            first_rc[0, :] = sign[0, :] * 3000
            first_rc[:, 0] = sign[:, 0] * 3000
            blocks.append(first_rc)
    for _ in range(600):
        blocks.append(rng.choice([-1, 1], (8, 8)) * rng.integers(0, 2000, (8, 8)))
    nat = np.stack(blocks).reshape(len(blocks), 64)
    zz = nat[:, zigzag].astype(np.int16).reshape(1, len(blocks), 64)
    for mode, param in (("none", 0.0), ("qtable", 0.0), ("divide", 3.0), ("divide", 0.37), ("divide", -41.5)):
        z = zz
        if mode == "qtable":
            z = np.clip(zz, -260, 260).astype(np.int16)     # keep z * q inside the int16-stream contract
        got, st = run_inverse(emul, z, mode, param)
        assert np.array_equal(got, oracle.inverse_i16(z, mode, param)), (mode, param)
        assert st[2] < 0.9, (mode, param, st[2])


@pytest.mark.parametrize("kind,limit", [("noise", 0.10), ("smooth", 0.02)])
def test_inverse_exact_tier_share(emul, kind, limit):
    """Census of the inverse exact tier on the bench's synthetic planes (JPEG table): the share of blocks
    that need the float64 tier, and bit-exactness of the two-tier result against the oracle."""
    from jpegx import synth
    a = synth.generate_plane(kind, 512, 512, seed=4)
    zz = oracle.forward_f32(a, "qtable")
    got, st = run_inverse(emul, zz, "qtable", 0.0)
    assert np.array_equal(got, oracle.inverse_i16(zz, "qtable"))
    assert st[1] / (a.size / 64) < limit
    assert st[2] < 0.9


def test_forward_bound_holds_on_adversarial_blocks(emul):
    """The per-coefficient forward bound F(k, l) u S / q is an L1 bound: it is approached when every sample
    pushes one coefficient in the same direction.  Blocks whose samples follow sign(C[k][i] C[l][n]) for every
    target coefficient (0 / 255 patterns, scaled and noisy versions, fractional and signed generic input): the
    observed fp32 error never reaches the bound and the two-tier result equals the oracle's."""
    C = oracle.tables()["dct_matrix"]
    rng = np.random.default_rng(11)
    blocks = []
    for k in range(8):
        for l in range(8):
            pos = np.outer(C[k], C[l]) > 0
            blocks.append(np.where(pos, 255.0, 0.0))
            blocks.append(np.where(pos, 255.0, 0.0) * (rng.random((8, 8)) > 0.1))
            blocks.append(np.where(pos, rng.integers(128, 256, (8, 8)), rng.integers(0, 128, (8, 8))).astype(float))
    for _ in range(400):
        blocks.append(rng.integers(0, 256, (8, 8)).astype(float))
    plane = np.hstack(blocks).astype(np.float32)
    worst = 0.0
    for mode, param in (("none", 0.0), ("qtable", 0.0), ("divide", 3.0), ("divide", 0.77), ("divide", -41.5)):
        for pixel in (1, 0):
            got, st = run_forward(emul, plane, mode, param, pixel)
            assert np.array_equal(got, oracle.forward_f32(plane, mode, param)), (mode, param, pixel)
            assert st[2] < 0.9, (mode, param, pixel, st[2])
            worst = max(worst, st[2])
    # generic input: quarter steps, signed, fractional (the non-pixel rounding counts)
    generic = np.hstack([b * s for b in blocks[:192] for s in (0.25, -1.0, 1.0 / 3.0)]).astype(np.float32)
    for mode, param in (("qtable", 0.0), ("divide", 2.0)):
        got, st = run_forward(emul, generic, mode, param, 0)
        assert np.array_equal(got, oracle.forward_f32(generic, mode, param))
        assert st[2] < 0.9, (mode, st[2])


def test_forward_exact_tier_share_with_the_per_coefficient_bound(emul):
    from jpegx import synth
    a = synth.generate_plane("noise", 512, 512, seed=9)
    _, st = run_forward(emul, a, "qtable", 0.0, 1)
    assert st[1] / (a.size / 64) < 0.03       # 3.5 % of noise blocks with the uniform 16 u S bound, ~2.3 % now


def test_bound_tables_in_the_header_cover_the_mechanical_derivation(emul):
    """The factors of the forward bound (15 levels per input kind), the weights of the inverse bound and the scale of
    the AAN transform's outputs, as compiled into the kernels (csrc/jpegx_math.h), against tests/derive_bounds.py, which
    runs the very flow graphs symbolically under the standard model of rounding: every table entry is at least what
    the derivation gives (a level may only round UP), and not wastefully more."""
    import derive_bounds as db
    emul.emul_aan_level_of.restype = ctypes.c_float
    emul.emul_inv_weight.restype = ctypes.c_float
    emul.emul_aan_g.restype = ctypes.c_double
    g, f_pixel, f_generic = db.forward_tables()
    assert np.allclose([emul.emul_aan_g(k) for k in range(8)], g, rtol=1e-15)
    assert np.allclose(AAN_G, g, rtol=1e-15)
    for pixel, want in ((1, f_pixel), (0, f_generic)):
        have = np.array([emul.emul_aan_level_of(n, pixel) for n in range(64)])
        assert np.all(have >= want - 1e-6), (pixel, np.argmax(want - have))
        assert np.all(have <= want * 1.35 + 1e-6)                       # 15 levels for 64 factors: little is given away
    w = db.inverse_plain_weights()
    have = np.array([emul.emul_inv_weight(n, 0) for n in range(64)])
    assert np.all(have >= w - 1e-9) and np.all(have <= w + 2.0 ** -12 + 1e-9)
    s = np.array([0.125 if k == 0 else 0.25 for k in range(8)])
    have2 = np.array([emul.emul_inv_weight(n, 2) for n in range(64)])
    assert np.allclose(have2 - have, 2 * np.outer(s, s).ravel(), atol=1e-7)
    # the hand-counted roundings of rounds 1-2 (jpegx_fwd_roundings / jpegx_idct8_roundings) were upper bounds of the same
    _, plain_pixel, plain_generic = db.forward_tables(db.dct8_plain)

    def hand(n, pix):
        def r(k, ex):
            return (0 if ex else 3) if k == 0 else ((5 if ex else 6) if k & 1 else ((2 if ex else 5) if k == 4 else (3 if ex else 5)))
        return r(n & 7, pix) + r(n >> 3, pix and (n & 7) == 0) + 1
    assert all(hand(n, True) >= plain_pixel[n] - 1e-9 and hand(n, False) >= plain_generic[n] - 1e-9 for n in range(64))
