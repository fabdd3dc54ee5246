"""What the sub-pixel tests share: the gather expectation of include/volpath.h's definition.

With factor S the sample of pixel (x, y) in frame f of a W x H image is the S = 1 sample of pixel (S x + i, S y + j) of the
S W x S H image, (i, j) = vp_subpixel_offset(x, y, f, S).  So an S-factor accumulator equals: every frame of the fine image
rendered on its own into a zeroed buffer (by the oracle, or by the library with S = 1), gathered at the offsets, and summed per
pixel in frame order in float32."""
import numpy as np


def offsets(volpath, W, H, frame, s):
    """(i, j) as (H, W) integer arrays, from the library's host function (needs no device)"""
    i = np.empty((H, W), np.intp)
    j = np.empty((H, W), np.intp)
    for y in range(H):
        for x in range(W):
            i[y, x], j[y, x] = volpath.subpixel_offset(x, y, frame, s)
    return i, j


def gather(volpath, fine, W, H, frame, s):
    """the W x H frame that factor s picks out of the (s H, s W, 4) frame `fine`"""
    assert fine.shape == (s * H, s * W, 4)
    i, j = offsets(volpath, W, H, frame, s)
    yy, xx = np.mgrid[0:H, 0:W]
    return fine[s * yy + j, s * xx + i]


def accumulate(volpath, W, H, s, first, n, fine_frame):
    """sum over frames first .. first+n-1 of the gathered fine frames, in frame order, float32; fine_frame(f) -> (s H, s W, 4)"""
    acc = np.zeros((H, W, 4), np.float32)
    for f in range(first, first + n):
        acc = acc + gather(volpath, fine_frame(f), W, H, f, s)
        assert acc.dtype == np.float32
    return acc


def fine_of(P, s):
    """the Param of the image the samples are computed on: P with (width, height) * s (a ctypes Param of the library or the oracle)"""
    F = type(P).from_buffer_copy(P)
    F.width, F.height = s * P.width, s * P.height
    return F


def library_fine_frames(vp, fineP):
    """fine_frame(f) through the library itself with S = 1: one frame at a time into a zeroed buffer"""
    buf = vp.DeviceBuffer(fineP.width, fineP.height)

    def frame(f):
        assert vp.get_subpixel() == 1
        buf.reset()
        vp.render_frames(buf.ptr, f, 1, fineP)
        return buf.download()
    return frame, buf


def library_expectation(vp, P, s, first, n):
    """the gather expectation from the library's own S = 1 renders of the fine image (current scene and modes); leaves the factor at s"""
    vp.set_subpixel(1)
    frame, buf = library_fine_frames(vp, fine_of(P, s))
    try:
        return accumulate(vp, P.width, P.height, s, first, n, frame)
    finally:
        buf.free()
        vp.set_subpixel(s)


def oracle_expectation(volpath, osc, oP, s, first, n):
    """the gather expectation from the CPU oracle's renders of the fine image; volpath: the module (for vp_subpixel_offset)"""
    fP = fine_of(oP, s)
    return accumulate(volpath, oP.width, oP.height, s, first, n, lambda f: osc.render_frame(fP, f, None)[0])
