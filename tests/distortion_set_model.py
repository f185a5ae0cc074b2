"""The NumPy twin of jpegx_picture_set_moments_n: the moments of tests/distortion_model.py per band, cut into n x n blocks and
laid behind each other in the STRIP order of tests/picture_set_model.py (picture-major, then band, then block-row-major inside
the band).  With colour the model pixels are tests/colour_model.py's YCbCr of the input.  A plain helper module of the suite;
tests/test_distortion_set_model.py holds the identity the set probe rests on against picture_set_model.pixels_twin."""
import numpy as np

import distortion_model
import picture_set_model


def moment_strips(pictures, bs, n, colour=0):
    """A list of uint8 [rows_p][cols_p][nb] -> (S1, S2, cnt), each int64 [nblk * n][n] in strip order."""
    out = ([], [], [])
    for px in pictures:
        model = picture_set_model.model_of(px, colour)
        for k in range(model.shape[2]):
            for acc, plane in zip(out, distortion_model.moments(model[:, :, k], bs, n)):
                acc.append(picture_set_model.blocks_of(plane, n))
    return tuple(np.concatenate(a).reshape(-1, n) for a in out)


def moments_twin(pictures, bs, n, colour=0):
    """uint64 [nblk * n][n]: the words of the device gather, S2 << 32 | S1."""
    s1, s2, _ = moment_strips(pictures, bs, n, colour)
    return distortion_model.pack(s1, s2)


def plane_sse(pictures, decoded, bs, n, colour=0):
    """int64 [nplanes]: per plane of the set the sum over its strip elements of S2 - 2 s S1 + cnt s^2 for a decoded strip s."""
    s1, s2, cnt = moment_strips(pictures, bs, n, colour)
    s = np.asarray(decoded).astype(np.int64).reshape(s1.shape)
    term = (s2 - 2 * s * s1 + cnt * s * s).reshape(-1, n * n).sum(axis=1)          # per block
    nb = pictures[0].shape[2]
    _, _, _, planes = picture_set_model.table_twin([p.shape[:2] for p in pictures], nb, bs, n)
    before = np.concatenate([[0], np.cumsum(term)])
    return before[planes[1:]] - before[planes[:-1]]
