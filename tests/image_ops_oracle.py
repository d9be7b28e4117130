"""trimSpatial (@Sources2D/Sources2D.m:942-965) restated in float64 with explicit shifts and a flood fill: no scipy.ndimage, so that it is independent of
cnmf_e_amd.hostops.trim_spatial, which it checks."""
import numpy as np


def _shifted(img, half, pad):
    """every translate of img by up to `half` in both directions, the image continued by `pad`"""
    d1, d2 = img.shape
    big = np.full((d1 + 2 * half, d2 + 2 * half), pad, dtype=np.float64)
    big[half:half + d1, half:half + d2] = img
    return [big[half + dr:half + dr + d1, half + dc:half + dc + d2] for dr in range(-half, half + 1) for dc in range(-half, half + 1)]


def imopen_square(img, sz):
    """imopen(img, strel('square', sz)), sz odd: imerode pads with +Inf, imdilate with -Inf"""
    assert sz % 2 == 1
    er = np.minimum.reduce(_shifted(img, sz // 2, np.inf))
    return np.maximum.reduce(_shifted(er, sz // 2, -np.inf))


def bwlabel4(bw):
    """bwlabel(bw, 4): labels in column-major order of each component's first pixel"""
    d1, d2 = bw.shape
    lab = np.zeros((d1, d2), dtype=np.int64)
    n = 0
    for c in range(d2):
        for r in range(d1):
            if bw[r, c] and not lab[r, c]:
                n += 1
                lab[r, c] = n
                stack = [(r, c)]
                while stack:
                    y, x = stack.pop()
                    for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
                        if 0 <= yy < d1 and 0 <= xx < d2 and bw[yy, xx] and not lab[yy, xx]:
                            lab[yy, xx] = n
                            stack.append((yy, xx))
    return lab


def trim_spatial(A, d1, d2, thr=0.01, sz=5, min_pixel=5):
    """A: dense d x K.  Returns (the trimmed d x K float64 matrix, ind_small)."""
    A = np.array(A, dtype=np.float64)
    ind_small = np.zeros(A.shape[1], dtype=bool)                         # :948
    for m in range(A.shape[1]):
        ai = A[:, m].copy()                                              # :950
        ai_open = imopen_square(ai.reshape(d1, d2, order="F"), sz)      # :951
        temp = ai_open > ai.max() * thr                                  # :953
        l = bwlabel4(temp).reshape(-1, order="F")                        # :954
        ind_max = int(np.argmax(ai_open.reshape(-1, order="F")))         # :955
        ai[l != l[ind_max]] = 0                                          # :957
        if np.count_nonzero(ai > 0) < min_pixel:                         # :958
            ind_small[m] = True
        A[:, m] = ai                                                     # :961
    return A, ind_small
