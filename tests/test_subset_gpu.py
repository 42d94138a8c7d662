"""GPU checks of the cohort subset (kernels_subset.hip, bann_genotypes_subset, bann_genotypes_fill_missing_a2).
The oracle is numpy (tests/subset_reference.py): g[np.ix_(markers, individuals)] of an int8 cohort with -1
for a missing call.  Every case compares the destination context with a second context that was loaded
directly with the expected subset through upload_bed, so every comparison is exact: the downloaded
genotypes, the missing counts, the statistics' bits, the bytes save_bed writes, and the bits of an LD band
and of a linear score, which read the rows' padding.  Cohorts are built as in test_ld_pairwise_gpu.py:
numpy, about 15 % of the calls missing, encode_bed_payload, keep_missing + upload_bed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import subset_reference as S

pytestmark = pytest.mark.gpu

E_SHAPE, E_STATE, E_ARG = -2, -4, -5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIP = int(re.search(r"#define SUBSET_STRIP (\d+)",
                      open(os.path.join(ROOT, "rs-bann_amd", "csrc", "bann_internal.h")).read()).group(1))


@pytest.fixture(scope="module")
def Ctx():
    from bann import BannContext
    return BannContext


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def loaded(Ctx, g, keep=True):
    """a context with the cohort g (int8, -1 missing) loaded through the .bed payload"""
    from bann.io import encode_bed_payload
    ctx = Ctx(0)
    if keep:
        ctx.keep_missing()
    ctx.upload_bed(encode_bed_payload(g), g.shape[1], g.shape[0])
    return ctx


def bed_bytes(ctx, tmp_path, name="x"):
    ctx.save_bed(str(tmp_path / name))
    return open(tmp_path / (name + ".bed"), "rb").read()


def assert_same_cohort(got, want, tmp_path, counts=True):
    """got and want are contexts: everything the library can say about their cohorts is equal"""
    assert (got.n, got.num_markers) == (want.n, want.num_markers)
    M = want.num_markers
    allm = np.arange(M)
    assert np.array_equal(got.download_genotypes(allm), want.download_genotypes(allm))
    if counts:
        assert np.array_equal(got.missing_counts(), want.missing_counts())
    for a, b in zip(got.genotype_stats(), want.genotype_stats()):
        assert np.array_equal(bits(a), bits(b))
    assert bed_bytes(got, tmp_path, "got") == bed_bytes(want, tmp_path, "want")
    # these two read the rows in 16-byte pieces, padding included
    if M >= 2:
        w = min(6, M - 1)
        assert np.array_equal(bits(got.ld_band(w)), bits(want.ld_band(w)))
    eff = np.random.default_rng(M).normal(size=M).astype(np.float32)
    assert np.array_equal(bits(got.linear_score([allm], eff)), bits(want.linear_score([allm], eff)))


def check_subset(Ctx, src, g, tmp_path, individuals=None, markers=None):
    want_g = S.subset(g, individuals, markers)
    with src.subset(individuals=individuals, markers=markers) as got, loaded(Ctx, want_g) as want:
        assert_same_cohort(got, want, tmp_path)
        assert np.array_equal(got.download_genotypes(np.arange(want_g.shape[0])), S.zero_coded(want_g))
        assert np.array_equal(got.missing_counts(), (want_g < 0).sum(axis=1))


# ------------------------------------------------------------------------------------------ geometry
@pytest.mark.parametrize("n_src", [63, 64, 65, 130, 257])
def test_row_geometry(Ctx, tmp_path, n_src):
    """M = 7; ascending lists of 1, 16, 17, 64 and 65 individuals (those that fit without a repeat: an
    ascending list is no longer than the cohort), everyone, everyone reversed, n_src + 3 draws with
    replacement, and a list from individual 0 to individual n_src - 1"""
    g = S.cohort(7, n_src, seed=n_src)
    rng = np.random.default_rng(1000 + n_src)
    lists = [np.sort(rng.choice(n_src, size=k, replace=False)) for k in (1, 16, 17, 64, 65) if k <= n_src]
    lists.append(np.arange(n_src))
    lists.append(np.arange(n_src)[::-1])
    lists.append(rng.integers(0, n_src, size=n_src + 3))
    inner = np.sort(rng.choice(np.arange(1, n_src - 1), size=n_src // 3, replace=False))
    lists.append(np.concatenate([[0], inner, [n_src - 1]]))
    with loaded(Ctx, g) as src:
        for ind in lists:
            check_subset(Ctx, src, g, tmp_path, individuals=ind)
        with src.subset(individuals=lists[0]) as got:
            assert got.subset_timing() > 0.0


def test_strip_seam(Ctx, tmp_path):
    """one individual more than a workgroup's strip holds: a strip boundary inside every row"""
    n_src = 9001
    g = S.cohort(3, n_src, seed=9)
    rng = np.random.default_rng(10)
    with loaded(Ctx, g) as src:
        check_subset(Ctx, src, g, tmp_path, individuals=np.sort(rng.choice(n_src, size=STRIP + 1, replace=False)))
        check_subset(Ctx, src, g, tmp_path, individuals=rng.integers(0, n_src, size=STRIP + 1))


def test_row_block(Ctx, tmp_path):
    """70 markers, a list of 37 of them, unsorted and with one repeat: individuals None, then both lists"""
    g = S.cohort(70, 65, seed=11)
    rng = np.random.default_rng(12)
    mk = rng.permutation(70)[:36]
    mk = np.insert(mk, 20, mk[3])
    assert mk.size == 37 and np.unique(mk).size == 36 and np.any(np.diff(mk) < 0)
    with loaded(Ctx, g) as src:
        check_subset(Ctx, src, g, tmp_path, markers=mk)
        check_subset(Ctx, src, g, tmp_path, individuals=rng.integers(0, 65, size=41), markers=mk)
        check_subset(Ctx, src, g, tmp_path, individuals=np.sort(rng.choice(65, size=33, replace=False)), markers=mk)


def test_both_none_is_a_copy(Ctx, tmp_path):
    g = S.cohort(7, 130, seed=13)
    with loaded(Ctx, g) as src, src.subset() as got:
        assert_same_cohort(got, src, tmp_path)
        assert np.array_equal(got.missing_counts(), (g < 0).sum(axis=1))


# ------------------------------------------------------------------------------------------ presence
def test_presence_rule(Ctx, tmp_path):
    from bann import BannError
    from bann.io import encode_bed_payload
    n = 70
    g = S.cohort(7, n, seed=14, missing=0.0)
    assert g.min() == 0
    gm = g.copy()
    gm[[0, 3, 6], 41] = -1                       # missing calls in individual 41 alone
    others = np.delete(np.arange(n), 41)
    with loaded(Ctx, gm) as src:
        with src.subset(individuals=others) as got, loaded(Ctx, g[:, others]) as want:
            assert np.array_equal(got.missing_counts(), np.zeros(7, np.int32))
            assert_same_cohort(got, want, tmp_path)
            assert bed_bytes(got, tmp_path)[3:] == encode_bed_payload(g[:, others])     # the complete data's bytes
        keep41 = np.array([5, 41, 69, 41])
        with src.subset(individuals=keep41) as got:
            assert got.missing_counts().tolist() == [2, 0, 0, 2, 0, 0, 2]
        check_subset(Ctx, src, gm, tmp_path, individuals=keep41)
    with loaded(Ctx, gm, keep=False) as src:
        with pytest.raises(BannError) as err:
            src.missing_counts()
        assert err.value.code == E_STATE
        with src.subset(individuals=keep41) as got, loaded(Ctx, S.subset(gm, keep41), keep=False) as want:
            with pytest.raises(BannError) as err:
                got.missing_counts()
            assert err.value.code == E_STATE
            assert_same_cohort(got, want, tmp_path, counts=False)


# -------------------------------------------------------------------------------------------- code 3
def test_code_three_flag_is_the_destinations(Ctx):
    """a single 3 at (marker 2, individual 5) and an fx-shaped branch over markers 0..8: the subset
    without individual 5 finalizes, the subset with it is refused as the source is"""
    from bann import BannError
    g = S.zero_coded(S.cohort(9, 40, seed=15, missing=0.0))
    g[2, 5] = 3
    snps = np.arange(9, dtype=np.int32)

    def finalize(ctx):
        ctx.add_branch(snps, [4, 4, 1], "tanh", "ridge_ard")
        ctx.finalize()
        assert ctx.kernel_path(0) == "fused"

    with Ctx(0) as src:
        src.upload_genotypes(g)
        without = np.delete(np.arange(40), 5)
        with src.subset(individuals=without) as got:
            assert np.array_equal(got.download_genotypes(snps), g[:, without])
            finalize(got)
        with src.subset(markers=[0, 1, 3, 4, 5, 6, 7, 8, 0]) as got:   # every individual, the marker dropped
            finalize(got)
        for kw in (dict(individuals=[7, 5, 9]), dict(markers=[8, 7, 6, 5, 4, 3, 2, 1, 0]), dict()):
            with src.subset(**kw) as got:
                assert int(got.download_genotypes(snps).max()) == 3
                with pytest.raises(BannError) as err:
                    finalize(got)
                assert err.value.code == E_ARG
        with pytest.raises(BannError) as err:
            finalize(src)
        assert err.value.code == E_ARG


# ---------------------------------------------------------------------------------- the source's state
def source_state(src, tmp_path):
    return (bed_bytes(src, tmp_path, "src"), [a.tobytes() for a in src.genotype_stats()],
            src.missing_counts().tobytes())


@pytest.mark.parametrize("finalized", [False, True])
def test_source_untouched(Ctx, tmp_path, finalized):
    g = S.cohort(12, 130, seed=16)
    rng = np.random.default_rng(17)
    with loaded(Ctx, g) as src:
        if finalized:
            src.add_branch(np.arange(12, dtype=np.int32), [4, 4, 1], "tanh", "ridge_ard")
            src.finalize(free_raw=False)
        before = source_state(src, tmp_path)
        check_subset(Ctx, src, g, tmp_path, individuals=rng.integers(0, 130, size=77))
        check_subset(Ctx, src, g, tmp_path, individuals=np.arange(3, 90), markers=[11, 0, 5])
        assert source_state(src, tmp_path) == before


def test_source_freed_is_refused(Ctx):
    from bann import BannError
    g = S.cohort(12, 65, seed=18)
    with loaded(Ctx, g) as src:
        src.add_branch(np.arange(12, dtype=np.int32), [4, 4, 1], "tanh", "ridge_ard")
        src.finalize(free_raw=True)
        with pytest.raises(BannError) as err:
            src.subset(individuals=[0, 1])
        assert err.value.code == E_STATE


def test_errors(Ctx, tmp_path):
    g = S.cohort(7, 65, seed=19)
    n, M = 65, 7

    def call(dst, src, ind, mk, n_keep=None, m_keep=None):
        """the C entry itself; n_keep / m_keep override the lists' lengths"""
        args = []
        for lst, count in ((ind, n_keep), (mk, m_keep)):
            a = None if lst is None else np.ascontiguousarray(lst, dtype=np.int64)
            args += [None if a is None else a.ctypes.data_as(C.POINTER(C.c_int64)),
                     count if count is not None else (0 if a is None else a.size)]
        return dst._lib.bann_genotypes_subset(dst._h, src._h, *args)

    with loaded(Ctx, g) as src, Ctx(0) as dst, loaded(Ctx, g[:3]) as fin:
        fin.add_branch(np.arange(3, dtype=np.int32), [4, 4, 1], "tanh", "ridge_ard")
        fin.finalize()
        assert call(src, src, [0, 1], None) == E_ARG                        # dst is src
        assert call(fin, src, [0, 1], None) == E_STATE                      # a finalized destination
        for bad, code in (([0, n], E_SHAPE), ([3, -1], E_SHAPE)):
            assert call(dst, src, bad, None) == code
            assert call(dst, src, bad, [0]) == code
        assert call(dst, src, None, [0, M]) == E_SHAPE
        assert call(dst, src, [1, 2], [M]) == E_SHAPE
        assert call(dst, src, [0, 1], None, n_keep=0) == E_ARG              # a list without entries
        assert call(dst, src, None, [0, 1], m_keep=0) == E_ARG
        assert call(dst, src, [0, 1], None, n_keep=-2) == E_ARG
        # the destination is as good as new, and a loaded one as it was
        ind = [64, 0, 7]
        assert call(dst, src, ind, None) == 0
        dst.n, dst.num_markers = 3, M
        with loaded(Ctx, S.subset(g, ind)) as want:
            assert_same_cohort(dst, want, tmp_path)
            assert call(dst, src, [0, n], None) == E_SHAPE
            assert_same_cohort(dst, want, tmp_path)
        # the Python method closes the context it made and raises
        from bann import BannError
        for kw, code in ((dict(individuals=[n]), E_SHAPE), (dict(individuals=[]), E_ARG), (dict(markers=[-1]), E_SHAPE)):
            with pytest.raises(BannError) as err:
                src.subset(**kw)
            assert err.value.code == code


# ---------------------------------------------------------------------------------------- downstream
def test_downstream_prediction(Ctx):
    """a subset finalized with two fx-shaped branches predicts, bit for bit, what the directly loaded
    cohort predicts with the same parameters"""
    g = S.cohort(40, 300, seed=20)
    rng = np.random.default_rng(21)
    ind = np.sort(rng.choice(300, size=203, replace=False))
    branches = [np.arange(0, 17, dtype=np.int32), np.arange(17, 40, dtype=np.int32)]
    rows = []
    with loaded(Ctx, g) as src, src.subset(individuals=ind) as got, loaded(Ctx, S.subset(g, ind)) as want:
        for ctx in (got, want):
            for snps in branches:
                ctx.add_branch(snps, [4, 4, 1], "tanh", "ridge_ard")
            ctx.finalize()
            prm = np.random.default_rng(22)
            out = []
            for b in range(2):
                assert ctx.kernel_path(b) == "fused"
                ctx.set_params(b, prm.normal(scale=0.5, size=ctx.num_params(b)).astype(np.float32))
                ctx.set_precisions(b, np.ones(ctx.num_precisions(b), np.float32))
                out.append(ctx.predict(b))
            rows.append(np.stack(out))
    assert rows[0].shape == (2, 203) and np.all(np.isfinite(rows[0])) and np.ptp(rows[0]) > 0
    assert np.array_equal(bits(rows[0]), bits(rows[1]))


# ----------------------------------------------------------------------------------- fill_missing_a2
def test_fill_missing_a2(Ctx, tmp_path):
    from bann import BannError
    from bann.io import encode_bed_payload
    g = S.cohort(9, 130, seed=23)
    assert (g < 0).sum() > 0
    filled = encode_bed_payload(S.zero_coded(g))
    with loaded(Ctx, g) as ctx, loaded(Ctx, g, keep=False) as plain:
        stats = [a.tobytes() for a in ctx.genotype_stats()]
        assert ctx.missing_counts().sum() == (g < 0).sum()
        assert bed_bytes(ctx, tmp_path)[3:] == encode_bed_payload(g)          # 01 where missing
        for _ in range(2):                                                   # the second call is a no-op
            ctx.fill_missing_a2()
            assert np.array_equal(ctx.missing_counts(), np.zeros(9, np.int32))
            assert [a.tobytes() for a in ctx.genotype_stats()] == stats
            assert bed_bytes(ctx, tmp_path) == bed_bytes(plain, tmp_path, "plain")
            assert bed_bytes(ctx, tmp_path)[3:] == filled
            assert np.array_equal(ctx.download_genotypes(np.arange(9)), S.zero_coded(g))
        plain.fill_missing_a2()                                              # keep off: nothing to do
        assert bed_bytes(plain, tmp_path, "plain")[3:] == filled
    with Ctx(0) as empty:
        with pytest.raises(BannError) as err:
            empty.fill_missing_a2()
        assert err.value.code == E_STATE
