"""csrc/moments.hip's two kernels on hand-made draws: draw_moments_kernel<PPT> (every compiled PPT: K = 2..8) and
corr_finalize_kernel, launched through the library's exported launchers on torch buffers of the test's own making, so that the
moment table between the two launches can be judged by itself.

Reference and bounds (tests/corr_cases.py, derived in its docstring, nothing measured): a = round5(x) - pivot in fp64, every sum
and the Pearson matrix in np.longdouble.  (a) the device's pair table: pivots array_equal round5 of draw 0, the count exactly nd,
pairs within (n + 1) 2^-53 sum |a_i a_j|, sums within (n + 1) 2^-53 sum |a_i|, all finite (the NaN padding beyond nd and the
other 2H - 1 forecast columns were not read); (b) corr_finalize_kernel array_equal -- NaN positions included -- with its fp64
restatement applied to the device's own table; (c) the matrix within E_ij / sqrt(c_ii c_jj) + |r| (rho_i / 2 + rho_j / 2 + 4 u),
times 1 + 2^-8, for every kind of hand-made column; (d) any split of the draws into blocks gives the bits of the single launch;
(e) constant and non-finite columns, nd = 1 and 2.  `mom` and `corr` carry a sentinel window before and after the block handed
to the kernels; every launch checks both.

Largest differences an MI355X run of this module showed, as |diff| / its bound.  Pair table: pairs 0.40, sums 0.25 (both at
nd = 3, where the bound is four roundings); per K = 2..8 pairs 0.30, 0.33, 0.33, 0.34, 0.40, 0.40, 0.39; at nd >= 127 pairs
below 0.08 and sums below 0.06 at every K, on the kinds pairs 0.080 (outlier, K = 8) and sums 0.085 (sticky, K = 8).
Correlations: 0.13 (6.1e-16 against 1.1e-14, K = 8, nd = 3); per K = 2..8 0.055, 0.099, 0.12, 0.085, 0.11, 0.13, 0.13, each at
nd = 3; 0.077 at nd = 2, 0.045 at most at nd = 63..65, 0.030 at nd = 127..200; per kind at nd = 129: plain 0.028, outlier 0.028
(4.1e-14 against 3.8e-12; its bounds reach 1.3e-11, rho 6.5e-12), collinear 0.025, duplicate 0.025, negated 0.028, sticky
0.038, constant 0.025.  Through the ABI (test_gpu_corr.py): 0.036 at most (K = 6), 0.011 at nrun = 1500, 0.033 on the streaming
route, the bounds there 1e-15 to 1.9e-11, no cell outside the guard.  The sums behind the bounds are worst cases over every sign
pattern, so one to two digits of slack at large n are their nature.  corr_finalize_kernel against its restatement, the
pivots, the count, NaN positions, symmetry, the diagonal and every block split: equal in every case."""
import numpy as np
import pytest

import corr_cases as cc

pytestmark = pytest.mark.gpu

SENTINEL = -7.25


class Device:
    """The launchers over torch buffers.  run(arrays, nd, K, H) -> (mom (W, stride), corr (W, NC, NC)) as numpy."""

    def __init__(self):
        import torch
        from hmc_jl_amd import _lib
        self.torch = torch
        self.lib = _lib.load()
        self.dev = torch.device("cuda", 0)

    def upload(self, a):
        return self.torch.from_numpy(np.array(a, dtype=np.float64, order="C")).to(self.dev)

    def tables(self, W, K):
        f64 = dict(dtype=self.torch.float64, device=self.dev)
        NC = cc.corr_columns(K)
        return (self.torch.full((W + 2, cc.moments_stride(K)), SENTINEL, **f64), self.torch.full((W + 2, NC, NC), SENTINEL, **f64))

    def accumulate(self, mom, arrays, nd, K, H, first):
        """One launch_moments over a block of draws: arrays in the ABI's layouts, their last axis the block's own nd_ld."""
        W, ld = arrays[0].shape[0], arrays[0].shape[-1]
        assert [a.shape for a in arrays] == [(W, K, ld)] * 3 + [(W, K * K, ld), (W, 2 * H, ld)] and 1 <= nd <= ld
        assert mom.shape == (W + 2, cc.moments_stride(K)) and mom.is_contiguous()
        t = [self.upload(a) for a in arrays]
        self.torch.cuda.synchronize(self.dev)
        cc.launch(self.lib, *[x.data_ptr() for x in t], mom[1:].data_ptr(), nd, ld, W, K, H, first)
        self.torch.cuda.synchronize(self.dev)

    def finish(self, mom, corr, W, K):
        assert corr.shape == (W + 2, cc.corr_columns(K), cc.corr_columns(K)) and corr.is_contiguous()
        self.torch.cuda.synchronize(self.dev)
        cc.finalize(self.lib, mom[1:].data_ptr(), corr[1:].data_ptr(), W, K)
        self.torch.cuda.synchronize(self.dev)
        m, c = mom.cpu().numpy(), corr.cpu().numpy()
        for a in (m, c):
            assert (a[0] == SENTINEL).all() and (a[-1] == SENTINEL).all(), "wrote outside its block"
        return m[1:-1], c[1:-1]

    def run(self, arrays, nd, K, H, blocks=None):
        """blocks: the draw counts of consecutive launches (default: one launch); each block is uploaded by itself, with its own
        leading dimension and base addresses, `first` on the first block only."""
        W = arrays[0].shape[0]
        mom, corr = self.tables(W, K)
        if blocks is None:
            self.accumulate(mom, arrays, nd, K, H, True)
        else:
            assert sum(blocks) == nd and all(b > 0 for b in blocks)
            d0 = 0
            for i, b in enumerate(blocks):
                pad = i % 3                                   # the leading dimension of a block need not be its draw count
                part = [np.concatenate([a[..., d0:d0 + b], np.full(a.shape[:-1] + (pad,), np.nan)], axis=-1) for a in arrays]
                self.accumulate(mom, part, b, K, H, i == 0)
                d0 += b
        return self.finish(mom, corr, W, K)


@pytest.fixture(scope="module")
def device(hmclib):
    return Device()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("K,nd,W,H,pad", cc.accumulation_cases())
def test_accumulation_and_finalisation(device, K, nd, W, H, pad):
    """(a) and (b), and the matrix against the reference as well."""
    arrays = cc.make_case(cc.case_seed(K, nd), W, K, H, nd, pad, "plain")
    cols = cc.columns(*arrays)
    ref = cc.reference(cols, nd)
    label = "K=%d (PPT %d) nd=%d W=%d H=%d pad=%d" % (K, cc.PPT_OF_K[K], nd, W, H, pad)
    mom, corr = device.run(arrays, nd, K, H)
    assert np.isfinite(mom).all(), (label, "a padding draw or another forecast column was read")
    cc.check_table(mom, ref, label)
    NC = cc.corr_columns(K)
    for w in range(W):
        want = cc.finalize_restated(mom[w], NC)
        assert np.array_equal(corr[w], want, equal_nan=True), (label, w, float(np.nanmax(np.abs(corr[w] - want))))
        assert np.array_equal(np.isnan(corr[w]), np.isnan(want))
    if nd > 1:
        assert np.isfinite(corr).all() and (np.einsum("wii->wi", corr) == 1.0).all() and (np.abs(corr) <= 1.0).all()
        assert np.array_equal(corr, np.swapaxes(corr, 1, 2))
    else:
        assert np.isnan(corr).all()                           # nd = 1: all NaN, diagonal included
    cc.check(corr, ref, label, constant=cc.constant_columns(cols, nd))
    if nd == 2:                                               # two draws: every correlation is +-1 within the bound
        tol = cc.tolerance(ref)["corr"]
        assert (np.abs(np.abs(corr) - 1.0) <= tol).all(), label


@pytest.mark.parametrize("kind,K,W,H,nd,pad", cc.kind_cases())
def test_kinds_end_to_end(device, kind, K, W, H, nd, pad):
    """(c), and of (e): duplicate columns give r <= 1 within the bound of 1, negated ones r >= -1 likewise; a constant column a
    NaN row and column."""
    arrays = cc.make_case(cc.case_seed(K, nd, kind), W, K, H, nd, pad, kind)
    cols = cc.columns(*arrays)
    ref = cc.reference(cols, nd)
    const = cc.constant_columns(cols, nd)
    label = "%s K=%d W=%d H=%d" % (kind, K, W, H)
    mom, corr = device.run(arrays, nd, K, H)
    cc.check_table(mom, ref, label)
    cc.check(corr, ref, label, constant=const)
    tol = cc.tolerance(ref)["corr"]
    if kind == "duplicate":
        assert (corr[:, 0, 1] <= 1.0).all() and (1.0 - corr[:, 0, 1] <= tol[:, 0, 1]).all()
    if kind == "negated":
        assert (corr[:, 0, 1] >= -1.0).all() and (corr[:, 0, 1] + 1.0 <= tol[:, 0, 1]).all()
    if kind == "constant":
        c = K + 1
        assert const[:, c].all() and np.isnan(corr[:, c, :]).all() and np.isnan(corr[:, :, c]).all()
        assert np.isfinite(np.delete(np.delete(corr, c, 1), c, 2)).all()


_SINGLE = {}


@pytest.mark.parametrize("K,nd,name", cc.split_cases())
def test_block_splits_give_the_same_bits(device, K, nd, name):
    """(d): the pair chains run in draw order whatever the blocks: the same `mom` bits and the same `corr` bits."""
    W, H = 2, 3
    arrays = cc.make_case(cc.case_seed(K, nd, "outlier"), W, K, H, nd, 0, "outlier")
    if (K, nd) not in _SINGLE:
        _SINGLE[K, nd] = device.run(arrays, nd, K, H)
        cc.check(_SINGLE[K, nd][1], cc.reference(cc.columns(*arrays), nd), "single launch K=%d nd=%d" % (K, nd))
    mom1, corr1 = _SINGLE[K, nd]
    blocks = cc.split_blocks(nd, name)
    assert len(blocks) >= 2 and sum(blocks) == nd
    mom, corr = device.run(arrays, nd, K, H, blocks=blocks)
    assert np.array_equal(bits(mom), bits(mom1)), (K, nd, name, "mom")
    assert np.array_equal(bits(corr), bits(corr1)), (K, nd, name, "corr")


@pytest.mark.parametrize("K", [3, 6])
def test_degenerate_columns_touch_only_their_own_cells(device, K):
    """(e): a constant column, then NaN and +Inf at draw 0, mid-chain and the last draw of one column: that column's row and
    column are NaN, every other cell has the bits of the clean run."""
    W, H, nd = 2, 3, 129
    clean_in = cc.make_case(cc.case_seed(K, nd), W, K, H, nd, 5, "plain")
    _, clean = device.run(clean_in, nd, K, H)
    assert np.isfinite(clean).all()
    NC = cc.corr_columns(K)

    def rest(a, c):
        return bits(np.delete(np.delete(a, c, 1), c, 2))

    def only_column(corr, c, label):
        assert np.isnan(corr[:, c, :]).all() and np.isnan(corr[:, :, c]).all(), label
        assert np.array_equal(rest(corr, c), rest(clean, c)), label

    for c in (1, 2 * K, NC - 1):                              # a mu, a pi and the forecast column
        arrays = [a.copy() for a in clean_in]
        col = cc.columns(*arrays)[:, c, :nd]                  # a copy: write through the arrays
        target = (arrays[0][:, 1], arrays[2][:, 0], arrays[4][:, 0])[(1, 2 * K, NC - 1).index(c)]
        assert np.array_equal(target[:, :nd], col)
        target[:, :nd] = 0.25 + 1e-7 * np.sin(np.arange(nd))          # constant after rounding
        _, corr = device.run(arrays, nd, K, H)
        only_column(corr, c, "constant column %d" % c)
        cols = cc.columns(*arrays)
        cc.check(corr, cc.reference(cols, nd), "constant column %d" % c, constant=cc.constant_columns(cols, nd))
        for where in (0, nd // 2, nd - 1):
            for bad in (np.nan, np.inf):
                target[:, :nd] = col
                target[:, where] = bad
                _, corr = device.run(arrays, nd, K, H)
                only_column(corr, c, "%s at draw %d of column %d" % (bad, where, c))
                cols = cc.columns(*arrays)
                cc.check(corr, cc.reference(cols, nd), "non-finite", constant=cc.constant_columns(cols, nd))
