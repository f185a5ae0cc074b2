"""The NumPy twin of jpegx_picture_set_blocks_u8 (csrc/jpegx_picture_set_u8.hip), the front of the dct_size-8 picture SET:
a list of uint8 pictures [rows_p][cols_p][nb] of unequal sizes -> the RAW uint8 block strip the uint8 forward kernels read.
Per picture the padded raw planes are tests/picture_gather_model.py's (the twin of the equal-size gather) on that picture
alone; each plane is cut into its R x R blocks, R = 8 * bs, block-row-major, and the blocks follow each other picture-major,
then band.  At block_size 2 and 4 block g is rows g * R .. g * R + R - 1 of a strip R bytes wide; at block_size 1 the strip is
16 bytes wide, block g at block row g // 2, column g % 2, and an odd block count is followed by one block of zeros.  A plain
helper module of the suite; tests/test_picture_set_8.py pins it to the reference's steps 0-3 without a device."""
import numpy as np

from picture_gather_model import planes_twin


def raw_blocks(pictures, bs, colour=0):
    """uint8 [T][R][R]: the set's blocks in strip order."""
    r = 8 * bs
    out = []
    for px in pictures:
        planes = planes_twin(np.asarray(px)[None], bs, colour)[0]          # [nb][H * bs][W * bs]
        nb, hh, ww = planes.shape
        out.append(planes.reshape(nb, hh // r, r, ww // r, r).transpose(0, 1, 3, 2, 4).reshape(-1, r, r))
    return np.concatenate(out)


def strip_of(blocks, bs):
    """[T][R][R] -> the strip as the forward kernel sees it: [T * R][R], or at block_size 1 [ceil(T / 2) * 8][16] with the pad."""
    t, r = blocks.shape[0], 8 * bs
    if bs != 1:
        return np.ascontiguousarray(blocks.reshape(t * r, r))
    if t % 2:
        blocks = np.concatenate([blocks, np.zeros((1, 8, 8), np.uint8)])
    return np.ascontiguousarray(blocks.reshape(-1, 2, 8, 8).transpose(0, 2, 1, 3).reshape(-1, 16))


def strip_twin_u8(pictures, bs, colour=0):
    return strip_of(raw_blocks(pictures, bs, colour), bs)
