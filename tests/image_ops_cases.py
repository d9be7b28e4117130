"""Seeded fp32 footprint sets for the image operations on single footprints (compactSpatial / circular, the 'dilate' search, trimSpatial): small fields of
view built around the places where a per-box kernel can go wrong.  case(name) -> dict(d1, d2, A (d1*d2 x K float32 CSC), nb, host_columns).  No video."""
import functools

import numpy as np
import scipy.sparse as sp

from cnmf_e_amd.engine import Engine

MAX_BOX = Engine.IMAGE_OPS_MAX_BOX
NAMES = ("blobs", "borders", "unchanged", "diagonal", "opening", "big_box", "nb2")


def _blob(d1, d2, r, c, sig_r, sig_c, amp, floor):
    y, x = np.mgrid[:d1, :d2]
    img = amp * np.exp(-0.5 * (((y - r) / sig_r) ** 2 + ((x - c) / sig_c) ** 2))
    img[img < floor] = 0
    return img


def _matrix(imgs, d1, d2):
    A = sp.csc_matrix(np.stack([np.asarray(i, dtype=np.float32).reshape(-1, order="F") for i in imgs], axis=1))
    A.eliminate_zeros(); A.sort_indices()
    assert A.dtype == np.float32 and A.shape == (d1 * d2, len(imgs))
    return A


def _blobs(seed=3):
    """1. Gaussian blobs with isolated speckles and single-pixel holes; the values span 1e-6 .. 1e3"""
    d1, d2 = 24, 20
    rng = np.random.default_rng(seed)
    imgs = []
    for k, amp in enumerate((1e3, 1.0, 1e-2, 30.0, 1e-3, 5.0)):
        r, c = rng.uniform(5, d1 - 5), rng.uniform(5, d2 - 5)
        img = _blob(d1, d2, r, c, rng.uniform(1.5, 3.0), rng.uniform(1.5, 3.0), amp, amp * 1e-3)
        img *= 1.0 + 0.2 * rng.uniform(-1, 1, img.shape)                 # (ragged: the gradient test has something to decide)
        nz = np.argwhere(img > 0)
        for i in rng.choice(len(nz), 3, replace=False):                 # single-pixel holes
            img[tuple(nz[i])] = 0
        zs = np.argwhere(img == 0)
        for i in rng.choice(len(zs), 6, replace=False):                 # isolated speckles, some of them tiny
            img[tuple(zs[i])] = amp * 10.0 ** rng.uniform(-3, -0.5)
        imgs.append(img)
    imgs[4] = np.maximum(imgs[4], (imgs[4] > 0) * 1e-6)                 # the smallest values of the set
    return d1, d2, imgs


def _borders():
    """2. footprints in a corner and along each border: the crop's edge is the field of view's, where erosion and dilation pad differently"""
    d1, d2 = 20, 18
    rng = np.random.default_rng(5)
    at = [(0, 0), (d1 - 1, d2 - 1), (0, d2 - 1), (d1 - 1, 0), (0, 9), (d1 - 1, 8), (10, 0), (9, d2 - 1), (1, 1)]
    imgs = []
    for r, c in at:
        img = _blob(d1, d2, r, c, 2.2, 2.6, 4.0, 4e-2) * (1.0 + 0.15 * rng.uniform(-1, 1, (d1, d2)))
        imgs.append(img)
    return d1, d2, imgs


def _unchanged():
    """3. columns that come back unchanged or empty: one-pixel-wide lines, a single pixel, an empty column, an all-equal plateau (first maximum, stable sort)"""
    d1, d2 = 12, 10
    line_v = np.zeros((d1, d2)); line_v[2:9, 4] = np.linspace(1, 2, 7)
    line_h = np.zeros((d1, d2)); line_h[6, 1:8] = np.linspace(2, 1, 7)
    single = np.zeros((d1, d2)); single[5, 5] = 3.0
    empty = np.zeros((d1, d2))
    plateau = np.zeros((d1, d2)); plateau[3:8, 2:8] = 0.75
    corner_single = np.zeros((d1, d2)); corner_single[0, 0] = 1.0
    return d1, d2, [line_v, line_h, single, empty, plateau, corner_single]


def _diagonal():
    """4. two lobes that touch only diagonally (4- against 8-connectivity); their energies differ by far more than 1 %"""
    d1, d2 = 16, 16
    imgs = []
    for amp2 in (0.5, 1.6):
        img = np.zeros((d1, d2))
        img[2:7, 2:7] = 1.0 + 0.1 * np.add.outer(np.arange(5), np.arange(5))
        img[7:12, 7:12] = amp2 * (1.0 + 0.1 * np.add.outer(np.arange(5), np.arange(5))[::-1, ::-1])
        imgs.append(img)
    gap = np.zeros((d1, d2)); gap[1:6, 1:6] = 2.0; gap[9:14, 9:14] = 1.0          # (three clear pixels between them: two components under either rule)
    imgs.append(gap)
    return d1, d2, imgs


def diagonal_lobe_energies():
    d1, d2, imgs = _diagonal()
    return [(float((i[:7, :7] ** 2).sum()), float((i[7:, 7:] ** 2).sum())) for i in imgs]


def _opening():
    """5. a thin footprint that imopen by 5 x 5 removes entirely (trimSpatial zeroes nothing), and one where the opening leaves a component that does not hold
    the raw maximum (a bright thin spur beside a dim plateau)"""
    d1, d2 = 22, 20
    thin = np.zeros((d1, d2)); thin[3:17, 6:8] = np.linspace(1, 3, 14)[:, None]
    spur = np.zeros((d1, d2)); spur[8:15, 3:10] = 1.0; spur[11, 10:17] = 10.0
    two = np.zeros((d1, d2)); two[2:8, 2:8] = 2.0; two[12:19, 11:18] = 3.0        # two openable components: only the brighter one stays
    return d1, d2, [thin, spur, two]


def _big_box():
    """6. an elongated dendrite, and ONE footprint whose bounding box alone has more cells than the device takes (two crossing diagonals): that column is the host's"""
    s = int(np.ceil(np.sqrt(MAX_BOX))) + 2
    d1, d2 = s + 8, s + 6
    dend = np.zeros((d1, d2))
    for i in range(50):
        dend[5 + i, 10 + i // 12:13 + i // 12] = 1.0 + 0.01 * i
    big = np.zeros((d1, d2))
    for i in range(s):
        big[3 + i, 2 + i] = 1.0 + 0.02 * i; big[3 + i, 3 + i] = 1.5; big[3 + i, 2 + s - i] = 0.8
    blob = _blob(d1, d2, 20.3, 40.6, 2.5, 2.0, 7.0, 7e-2)
    assert s * s > MAX_BOX
    return d1, d2, [dend, big, blob]


@functools.lru_cache(maxsize=None)
def case(name):
    make = {"blobs": _blobs, "borders": _borders, "unchanged": _unchanged, "diagonal": _diagonal, "opening": _opening, "big_box": _big_box, "nb2": _blobs}[name]
    d1, d2, imgs = make(11) if name == "nb2" else make()
    A = _matrix(imgs, d1, d2)
    A.data.setflags(write=False)
    return dict(d1=d1, d2=d2, A=A, nb=2 if name == "nb2" else 1, host_columns=1 if name == "big_box" else 0)
