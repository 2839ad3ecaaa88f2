"""The numpy references of tests/evalkern_ref.py pinned to what already exists (scipy, Pillow and the
float64 oracle), and the premises of the GPU cases of tests/test_gpu_evalkern.py: on the very input a
case hands the kernel, the transposed or mis-strided variant of the reference differs from the
reference, so that the case cannot pass vacuously. The variants run on the host only. No GPU."""
import types

import numpy as np
import pytest

from tests import analyzer_ref as A
from tests import evalkern_ref as R

F32, F64 = np.float32, np.float64


def differs(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape != b.shape or not np.array_equal(R.bits(a), R.bits(b))


def host_layout(name, extra_slot=False):
    """(band offsets, pos int32, cells = AH * AW, mask_len) of a COEFF_PLANS entry without a device:
    the band shapes of band_layout through the project's coeff_array_layout."""
    from wam_amd.evalcore import coeff_array_layout
    _, L, hw, J = R.COEFF_PLANS[name]
    shapes, off = R.band_layout(hw, L, J)
    pos, shape = coeff_array_layout(types.SimpleNamespace(band_shapes=shapes, levels=J))
    cells = shape[0] * shape[1]
    pos = pos.astype(np.int32)
    if extra_slot:
        return off, R.extra_slot_pos(pos, cells), cells, cells + 1
    return off, pos, cells, cells


# ------------------------------------------------------------------------------ pins
@pytest.mark.parametrize("shape,sigma,radius", [((224, 224), 2, 8), ((5, 37), 2, 8), ((37, 5), 2, 8), ((3, 3), 2, 8),
                                                ((1, 9), 2, 8), ((9, 1), 2, 8), ((40, 56), 2, 8), ((17, 64), 0.5, 2),
                                                ((8, 12), 8, 32)])
def test_gaussian_ref_is_scipy_bit_for_bit(shape, sigma, radius):
    from scipy.ndimage import gaussian_filter
    x = R.gauss_input(2, shape[0], shape[1], seed=3)
    w, r = R.gaussian_weights(sigma)
    assert r == radius and w.shape == (r + 1,)
    got = R.gaussian_ref(x, w, r)
    for i in range(2):
        R.assert_bits(got[i], gaussian_filter(x[i], sigma=sigma), "gaussian_ref %s sigma %s" % (shape, sigma))


def test_symmetric_index_reflects_any_number_of_times():
    ext = np.array([R.symmetric_index(i, 3) for i in range(-9, 12)])
    assert np.array_equal(ext, [2, 1, 0, 0, 1, 2, 2, 1, 0, 0, 1, 2, 2, 1, 0, 0, 1, 2, 2, 1, 0])
    assert np.array_equal(R.symmetric_index(np.arange(-70, 70), 1), np.zeros(140))


@pytest.mark.parametrize("n_iter", [8, 7])
def test_rank_masks_ref_vs_oracle(n_iter):
    from oracle import evaluation_ref as E
    wam = np.random.RandomState(n_iter).standard_normal((37, 52))
    assert np.unique(wam).size == wam.size
    order = np.argsort(wam, axis=None)[::-1]
    rank = np.empty(wam.size, dtype=np.int32)
    rank[order] = np.arange(wam.size)
    ins, dele = E.generate_masks(n_iter, wam)
    n_comp = int(wam.size / n_iter)
    R.assert_bits(R.rank_masks_ref(rank, n_iter, n_comp, wam.size, 0), ins.reshape(n_iter + 1, -1).astype(F32), "ins")
    R.assert_bits(R.rank_masks_ref(rank, n_iter, n_comp, wam.size, 1), dele.reshape(n_iter + 1, -1).astype(F32), "del")


@pytest.mark.parametrize("name", list(R.COEFF_PLANS))
def test_band_layout_and_coeff_masks_ref_vs_oracle(name):
    """band_layout == the shapes of oracle.dwt.wavedec2 (symmetric); coeff_masks_ref of one plane ==
    (coeffs_to_array * mask) read back at the coefficients' positions, in float32."""
    from oracle import dwt, evaluation_ref as E
    wav, L, hw, J = R.COEFF_PLANS[name]
    c = dwt.wavedec2(np.random.RandomState(2).standard_normal(hw), wav, J, mode="symmetric")
    bands = [c[0]] + [t for lv in c[1:] for t in lv]
    shapes, off = R.band_layout(hw, L, J)
    assert [b.shape for b in bands] == shapes
    want = {"db4_37x52_J2": [252, 638], "db2_40x56_J2": [192, 609], "haar_24x40_J3": [15, 60, 240],
            "sym4_33x20_J1": [260]}[name]
    assert sorted(set(np.diff(off))) == want
    off2, pos, cells, mask_len = host_layout(name)
    assert off2 == off and np.unique(pos).size == pos.size == off[-1]
    arr, _ = E.coeffs_to_array(c)
    assert arr.size == cells
    mask = np.random.RandomState(3).uniform(-2, 2, (2,) + arr.shape).astype(F32)
    flat = np.concatenate([b.reshape(-1) for b in bands]).astype(F32)
    got = R.coeff_masks_ref(off, 1, flat, pos, 2, mask_len, mask)
    for m in range(2):
        prod = (arr.astype(F32) * mask[m]).reshape(-1)[pos]
        ref = np.concatenate([got[2 * off[b] + m * (off[b + 1] - off[b]):2 * off[b] + (m + 1) * (off[b + 1] - off[b])]
                              for b in range(len(off) - 1)])
        R.assert_bits(ref, prod, "coeff_masks_ref %s mask %d" % (name, m))


def test_masked_sums_ref_vs_oracle():
    """binary subsets on a ragged map: fsum against sum_importance's np.sum to 1e-13; S_m is the sum of
    magnitudes."""
    import random
    from oracle import evaluation_ref as E
    rng = np.random.RandomState(4)
    wam = rng.standard_normal((37, 52))
    random.seed(5)
    idx = E.generate_subsets(7, 20, 6)
    sub = np.zeros((6, 7, 7), dtype=F32)
    for j, s in enumerate(idx):
        cx, cy = zip(*s)
        sub[j, cx, cy] = 1
    cell = R.upsample_ref(np.arange(49, dtype=F32).reshape(1, 7, 7), (37, 52))[0].astype(np.int64)
    sums, mags = R.masked_sums_ref(wam, sub, cell)
    assert np.allclose(sums, E.sum_importance(wam, idx, 7, 6), rtol=1e-13, atol=0)
    assert np.allclose(mags, E.sum_importance(np.abs(wam), idx, 7, 6), rtol=1e-13, atol=0) and (mags >= np.abs(sums)).all()


@pytest.mark.parametrize("hw", [(224, 224), (97, 61)])
def test_pil_resize_ref_vs_to_input(hw):
    """at 224^2 the resize is the identity: pil_resize_ref == analyzer_ref.to_input (torch's ToTensor +
    Normalize) bit for bit; from another size both go through the real Pillow."""
    u8 = np.random.RandomState(6).randint(0, 256, (2, 3) + hw).astype(np.uint8)
    got = R.pil_resize_ref(u8, (224, 224), A.IMAGENET_MEAN, A.IMAGENET_STD)
    for i in range(2):
        R.assert_bits(got[i], A.to_input(np.ascontiguousarray(np.moveaxis(u8[i], 0, 2))).numpy(), "pil_resize_ref %d" % i)


# ------------------------------------------------------------------------------ premises: gaussian
@pytest.mark.parametrize("items,h,w,sigma", R.GAUSS_CASES)
def test_premise_gaussian(items, h, w, sigma):
    x = R.gauss_input(items, h, w)
    wt, r = R.gaussian_weights(sigma)
    assert r <= 64
    ref = R.gaussian_ref(x, wt, r)
    assert np.isfinite(ref).all()
    if h != w:
        swapped = R.gaussian_ref(x.reshape(items, w, h), wt, r).reshape(items, h, w)
        assert differs(swapped, ref), "h and w swapped goes unseen"
    if min(h, w) > 1 or h != w:
        for axes in ((0, 0), (1, 1)):
            assert differs(R.gaussian_ref(x, wt, r, axes=axes), ref), "both passes along axis %d go unseen" % axes[0]
    if items > 1:
        stride0 = R.gaussian_ref(np.broadcast_to(x[:1], x.shape), wt, r)
        assert all(differs(stride0[i], ref[i]) for i in range(1, items)), "item stride 0 goes unseen"
    if (h, w, sigma) == (8, 12, 8):
        assert r == 32 > 2 * max(h, w)
    if sigma == 16:
        assert r == 64


# ------------------------------------------------------------------------------ premises: ranking masks
@pytest.mark.parametrize("length,n_iter,n_comp", R.RANK_CASES)
def test_premise_rank_cases(length, n_iter, n_comp):
    perm, rep = R.rank_rows(length)
    assert np.array_equal(np.sort(perm), np.arange(length))
    assert length < 3 or np.unique(rep).size < length
    ins = R.rank_masks_ref(perm, n_iter, n_comp, length, 0)
    count = ins.sum(axis=1)
    assert count[0] == 0 and count[-1] == length
    want = [min(m * n_comp, length) for m in range(n_iter)] + [length]
    assert np.array_equal(count, want)
    if (length, n_iter) == (1924, 8):
        assert count[n_iter - 1] < length - n_comp       # only the forced last mask is full
    if (length, n_iter) == (5, 8):
        assert not ins[:8].any() and ins[8].all()
    if (length, n_iter) == (100, 4):
        assert 2 * n_comp > length and count[2] == count[3] == length
    assert np.array_equal(R.rank_masks_ref(perm, n_iter, n_comp, length, 1), 1 - ins)
    if length > 5 and n_iter > 1:
        assert differs(R.rank_masks_ref(rep, n_iter, n_comp, length, 0), ins)


# ------------------------------------------------------------------------------ premises: coefficient masks
@pytest.mark.parametrize("extra_slot", [False, True])
@pytest.mark.parametrize("n_masks", [1, 5, 17])
@pytest.mark.parametrize("items", [1, 3])
@pytest.mark.parametrize("name", list(R.COEFF_PLANS))
def test_premise_coeff_masks(name, items, n_masks, extra_slot):
    off, pos, cells, mask_len = host_layout(name, extra_slot)
    K = off[-1]
    coeffs, masks = R.coeff_input(off, items, n_masks, pos, mask_len)
    ref = R.coeff_masks_ref(off, items, coeffs, pos, n_masks, mask_len, masks)
    assert ref.size == n_masks * items * K and not (ref == F32(R.SENTINEL)).any()
    # the NaN coefficient under every mask, inf * 0 where a mask (mask 0 for one) is zero at the inf
    # coefficient; +-inf where it is not
    zeros_at_inf = int((masks[:, pos[off[-2] + 3]] == 0).sum())
    assert zeros_at_inf >= 1 and np.isnan(ref).sum() == n_masks + zeros_at_inf
    assert np.isinf(ref).sum() == n_masks - zeros_at_inf >= (n_masks > 1)
    assert (masks == 0).sum() > 2 * n_masks and np.signbit(masks[masks == 0]).any() and (masks == 1).any()
    if extra_slot:
        share = (pos == cells).mean()
        assert 0.02 < share < 0.09 and mask_len == cells + 1
    if n_masks > 1:
        wrong = R.coeff_masks_ref(off, items, coeffs, pos, n_masks, mask_len, masks, out_band_items=items)
        assert differs(wrong, ref), "`items` where n_masks * items belongs goes unseen"
        wrong = R.coeff_masks_ref(off, items, coeffs, pos, n_masks, mask_len, masks, mask_stride=mask_len - 1)
        assert differs(wrong, ref), "mask_len without the extra slot goes unseen"
        first = np.broadcast_to(masks[:1], masks.shape)
        assert differs(R.coeff_masks_ref(off, items, coeffs, pos, n_masks, mask_len, first), ref), "mask stride 0"
    if items > 1:
        plane0 = np.concatenate([np.tile(coeffs[items * off[b]:items * off[b] + off[b + 1] - off[b]], items)
                                 for b in range(len(off) - 1)])
        assert differs(R.coeff_masks_ref(off, items, plane0, pos, n_masks, mask_len, masks), ref), "item stride 0"


@pytest.mark.parametrize("name", list(R.COEFF_PLANS))
def test_premise_coeff_positions_are_not_symmetric(name):
    """the array of every plan is non-square: positions built with the row stride of the transposed array
    differ, and leave the array."""
    from wam_amd.evalcore import coeff_array_layout
    _, L, hw, J = R.COEFF_PLANS[name]
    shapes, _ = R.band_layout(hw, L, J)
    pos, shape = coeff_array_layout(types.SimpleNamespace(band_shapes=shapes, levels=J))
    assert shape[0] != shape[1]
    rows, cols = pos // shape[1], pos % shape[1]
    assert differs(rows * shape[0] + cols, pos)


# ------------------------------------------------------------------------------ premises: superpixel masks
@pytest.mark.parametrize("grid,hw", R.ZOOM_CASES)
def test_premise_upsample(grid, hw):
    g = R.grid_masks(4, grid)
    ref = R.upsample_ref(g, hw)
    assert np.signbit(ref).any() and not np.signbit(ref).all() and np.unique(g).size == g.size
    if hw[0] != hw[1]:
        swapped = R.upsample_ref(g, hw[::-1]).reshape(4, -1)
        assert differs(swapped, ref.reshape(4, -1)), "h and w swapped goes unseen"
    assert all(differs(ref[m], ref[0]) for m in range(1, 4)), "mask stride 0 goes unseen"


@pytest.mark.parametrize("n_masks", [1, 16])
@pytest.mark.parametrize("length,hw,grid", R.SUMS_CASES)
def test_premise_masked_sums(length, hw, grid, n_masks):
    assert hw[0] * hw[1] == length
    wam, g = R.sums_input(length, n_masks, grid)
    cell = R.upsample_ref(np.arange(grid * grid, dtype=F32).reshape(1, grid, grid), hw)[0].astype(np.int64)
    assert np.unique(g[1:]).size > 2 or n_masks == 1
    pos, mags_pos = R.masked_sums_ref(wam[0], g, cell)
    mixed, mags = R.masked_sums_ref(wam[1], g, cell)
    assert (wam[1] > 0).any() and (wam[1] < 0).any()
    assert abs(mixed[0]) <= 1e-9 * mags[0]          # near zero next to S_0: the bound is about S_m
    assert abs(pos[0]) == pytest.approx(mags_pos[0], rel=1e-12)
    if n_masks > 1:
        assert np.unique(pos).size == n_masks       # mask stride 0 would repeat mask 0's sum


# ------------------------------------------------------------------------------ premises: Pillow resample
@pytest.mark.parametrize("rule", [0, 1])
@pytest.mark.parametrize("src,size", R.RESIZE_CASES)
def test_premise_resize(src, size, rule):
    from wam_amd.evalcore import pil_bilinear_coeffs
    (rh, rw), (oh, ow) = src, size
    arms = {(100, 224): (None, 3), (300, 224): (None, 5), (512, 512): (7, 7), (50, 120): (13, 9), (97, 61): (3, 3)}[src]
    assert (rw == ow) == (arms[0] is None) and rh != oh
    if arms[0] is not None:
        assert pil_bilinear_coeffs(rw, ow)[0] == arms[0]
    assert pil_bilinear_coeffs(rh, oh)[0] == arms[1]
    rec = R.resize_input(rh, rw, rule)
    u8, _ = A.quantize_ref(rec, rule)
    assert np.unique(u8[1]).size == 1 and np.unique(u8[0]).size > 200
    u8 = u8.reshape(3, 3, rh, rw)
    ref = R.pil_resize_ref(u8, size, A.IMAGENET_MEAN, A.IMAGENET_STD)
    assert ref.shape == (3, 3, oh, ow) and np.unique(ref[1, 0]).size == 1
    if rh != rw:
        swapped = R.pil_resize_ref(u8.reshape(3, 3, rw, rh), size, A.IMAGENET_MEAN, A.IMAGENET_STD)
        assert differs(swapped, ref), "h and w swapped goes unseen"
    assert differs(ref[2], ref[0]), "image stride 0 goes unseen"
    chan0 = R.pil_resize_ref(np.repeat(u8[:, :1], 3, axis=1), size, A.IMAGENET_MEAN, A.IMAGENET_STD)
    assert differs(chan0, ref), "channel stride 0 goes unseen"
