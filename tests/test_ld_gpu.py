"""GPU checks of the LD band, the LD graph and group-by-ld (kernels_ld.hip, bann_ld.hip): the band is
bit-equal to the integer restatement of tests/ld_reference.py, the graph equals its edge set, and the
grouping built from it trains a branch.  The contexts hold genotypes only unless a test says otherwise."""
import functools
import os

import numpy as np
import pytest

import bann_oracle as O
import ld_reference as R
from helpers import f32_branch, norm_rel, x_std

pytestmark = pytest.mark.gpu

PLINK = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plink")


@pytest.fixture(scope="module")
def Ctx():
    from bann import BannContext
    return BannContext


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_band_equal(got, want):
    assert got.shape == want.shape and got.dtype == np.float32
    bad = np.argwhere(bits(got) != bits(want))
    assert bad.size == 0, (len(bad), bad[:5].tolist(), [(got[tuple(b)], want[tuple(b)]) for b in bad[:5]])


@functools.lru_cache(maxsize=None)
def cohort(name):
    """the test cohorts, [M][n] int8, built once"""
    if name == "small":
        return O.bed_decode(open(os.path.join(PLINK, "small.bed"), "rb").read()[3:], 20, 11)
    if name == "random":
        return O.bed_decode(open(os.path.join(PLINK, "random.bed"), "rb").read()[3:], 100, 20)
    if name == "blocks":  # n = 3 * 64 + 1; 300 markers: 27 blocks of 10, one singleton after each, 3 more at the end
        return R.ld_block_cohort(np.random.default_rng(5), 193, 27, 10, 30)
    if name == "deep":    # many K steps; marker 30 is all 2s (zero variance) beside markers with v > 0
        g = R.ld_block_cohort(np.random.default_rng(6), 4099, 7, 9, 7)
        g[30, :] = 2
        return g
    if name == "groups":  # the grouping cohort: n = 257, 6 blocks of 9 plus 3 singletons
        return R.ld_block_cohort(np.random.default_rng(7), 257, 6, 9, 3)
    if name == "dups":    # exact duplicate columns: 5 = 3, 6 = 3, 40 = 38
        g = R.ld_block_cohort(np.random.default_rng(8), 130, 5, 9, 5).copy()
        g[5] = g[3]
        g[6] = g[3]
        g[40] = g[38]
        return g
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def ref_band(name, window):
    b = R.band(cohort(name), window)
    b.setflags(write=False)
    return b


def context(Ctx, name):
    ctx = Ctx(0)
    if name in ("small", "random"):
        ctx.load_bed(os.path.join(PLINK, name))
    else:
        ctx.upload_genotypes(cohort(name))
    return ctx


@pytest.mark.parametrize("name,window", [("small", 10), ("random", 3), ("random", 25), ("blocks", 137), ("deep", 69)])
def test_band_bit_equal(Ctx, name, window):
    g = cohort(name)
    want = ref_band(name, window)
    r2 = R.r2_matrix(g)
    x = g.astype(np.int64)
    v = g.shape[1] * (x * x).sum(axis=1) - x.sum(axis=1) ** 2
    if name == "small":  # one zero-variance marker; 4 pairs at r2 >= 0.2
        assert int((v == 0).sum()) == 1
        z = int(np.flatnonzero(v == 0)[0])
        assert np.all(r2[z] == 0) and np.all(r2[:, z] == 0)
        assert len(R.edges(g, 10, 0.2)) == 4
    if name == "deep":
        assert v[30] == 0 and v[29] > 0 and v[31] > 0 and np.all(want[30] == 0)
    if name == "blocks":  # the comparison is not one of zeros
        assert len(R.edges(g, window, 0.5)) >= 100
    with context(Ctx, name) as ctx:
        got = ctx.ld_band(window)
        assert ctx.ld_timing() > 0.0
    if window >= g.shape[0]:  # tail entries past the last marker are 0
        assert np.all(got[:, g.shape[0] - 1:] == 0)
    assert_band_equal(got, want)


def test_band_chunked_retrieval(Ctx):
    g = cohort("blocks")
    M, window = g.shape[0], 137
    want = ref_band("blocks", window)
    with context(Ctx, "blocks") as ctx:
        whole = ctx.ld_band(window, 0, M)
        assert_band_equal(whole, want)
        sevens = np.concatenate([ctx.ld_band(window, f, min(7, M - f)) for f in range(0, M, 7)])
        assert_band_equal(sevens, want)
        for f in (0, 1, 63, 64, 127, 128, 200, M - 1):  # chunk size 1, at and around the tile edges
            assert_band_equal(ctx.ld_band(window, f, 1), want[f:f + 1])
        assert ctx.ld_band(window, M, 0).shape == (0, window)


def graph_edges(ctx, *args, **kw):
    off, nb = ctx.ld_graph(*args, **kw)
    assert off.dtype == np.int64 and nb.dtype == np.int32 and off[0] == 0 and off[-1] == nb.size
    return R.csr_edges(off, nb)


def test_graph_equals_edge_set(Ctx):
    g = cohort("blocks")
    with context(Ctx, "blocks") as ctx:
        for window, thr in [(137, 0.2), (137, 0.5), (5, 0.5), (40, 0.2)]:
            want = R.edges(g, window, thr)
            assert len(want) >= 100
            assert graph_edges(ctx, window, thr) == want


def test_graph_threshold_tie_on_duplicates(Ctx):
    """r2_min = 1.0: cov^2 = v_j v_k as integers for exact duplicates, so they and only they are edges"""
    g = cohort("dups")
    want = R.edges(g, 20, 1.0)
    assert want == {(3, 5), (3, 6), (5, 6), (38, 40)}
    with context(Ctx, "dups") as ctx:
        assert graph_edges(ctx, 20, 1.0) == want


def test_graph_chrom_bp_filter(Ctx):
    """two chromosomes split inside a block, and a max_bp that cuts inside the blocks"""
    g = cohort("blocks")
    M = g.shape[0]
    chrom = (np.arange(M) >= 104).astype(np.int32)   # marker 104 is inside the block 99 .. 108
    bp = (1000 * np.arange(M)).astype(np.int64)
    with context(Ctx, "blocks") as ctx:
        for max_bp in (0, 4500):
            want = R.edges(g, 137, 0.5, chrom, bp, max_bp)
            free = R.edges(g, 137, 0.5)
            assert 0 < len(want) < len(free)
            assert graph_edges(ctx, 137, 0.5, chrom=chrom, bp=bp, max_bp=max_bp) == want
        with pytest.raises(ValueError):
            ctx.ld_graph(137, 0.5, chrom=chrom)


def test_results_do_not_depend_on_the_marker_blocks(Ctx):
    """an S-band limit that holds 128 rows of a 137-marker window: the 300 markers go in three blocks
    (the default limit takes every cohort here in one); band, pieces that start inside a block, graph
    and filtered graph are what the one-block calls give"""
    from bann import BannError
    g = cohort("blocks")
    M, window = g.shape[0], 137
    want = ref_band("blocks", window)
    chrom = (np.arange(M) >= 104).astype(np.int32)
    bp = (1000 * np.arange(M)).astype(np.int64)
    with context(Ctx, "blocks") as ctx:
        ctx.ld_scratch_limit(128 * window * 4)
        assert_band_equal(ctx.ld_band(window), want)
        assert_band_equal(ctx.ld_band(window, 100, 200), want[100:300])   # blocks 100..227, 228..299
        assert graph_edges(ctx, window, 0.5) == R.edges(g, window, 0.5)
        assert graph_edges(ctx, window, 0.5, chrom=chrom, bp=bp, max_bp=4500) == R.edges(g, window, 0.5, chrom, bp, 4500)
        ctx.ld_scratch_limit(128 * (M - 1) * 4)                            # a window clipped to M - 1: three blocks too
        assert_band_equal(ctx.ld_band(400), R.band(g, 400))
        ctx.ld_scratch_limit(128 * 5 * 4)                                  # room for a window of 5 only
        assert graph_edges(ctx, 5, 0.5) == R.edges(g, 5, 0.5)
        with pytest.raises(BannError) as e:
            ctx.ld_band(window)
        assert e.value.code == -5
        with pytest.raises(BannError) as e:
            ctx.ld_scratch_limit((128 << 20) + 1)
        assert e.value.code == -5
        ctx.ld_scratch_limit(0)                                            # the default again
        assert_band_equal(ctx.ld_band(window), want)


def test_state_errors(Ctx):
    from bann import BannError
    g = cohort("groups")
    snps = np.arange(9, dtype=np.int32)
    with Ctx(0) as ctx:
        with pytest.raises(BannError) as e:   # before any genotypes
            ctx.ld_band(5)
        assert e.value.code == -4
        ctx.upload_genotypes(g)
        for w in (0, -3):
            with pytest.raises(BannError) as e:
                ctx.ld_band(w)
            assert e.value.code == -5
            with pytest.raises(BannError) as e:
                ctx.ld_graph(w)
            assert e.value.code == -5
        ctx.add_branch(snps, [2, 1, 1])
        ctx.finalize(free_raw=False)
        assert_band_equal(ctx.ld_band(40), ref_band("groups", 40))
    with Ctx(0) as ctx:
        ctx.upload_genotypes(g)
        ctx.add_branch(snps, [2, 1, 1])
        ctx.finalize(free_raw=True)
        with pytest.raises(BannError) as e:
            ctx.ld_band(40)
        assert e.value.code == -4
        with pytest.raises(BannError) as e:
            ctx.ld_graph(40)
        assert e.value.code == -4


def test_group_by_ld_end_to_end(Ctx, tmp_path):
    """cohort -> LD graph -> centered grouping -> .groups file -> branches -> one forward"""
    from bann.io import group_by_ld, read_grouping, write_grouping
    g = cohort("groups")
    M, n = g.shape
    for window in (5, 40):
        assert len(R.edges(g, window, 0.5)) >= 100
    want, want_un = R.centered(R.adjacency(M, R.edges(g, 40, 0.5)), 1)
    assert sum(len(x) >= 3 for x in want) >= 1
    rng = np.random.default_rng(11)
    with context(Ctx, "groups") as ctx:
        groups, ungrouped = group_by_ld(ctx, 40, 0.5, 1)
        assert [x.tolist() for x in groups] == want and ungrouped == want_un
        path = str(tmp_path / "cohort.groups")
        write_grouping(path, groups)
        back = read_grouping(path)
        assert [x.tolist() for x in back] == want
        branches = []
        for snps in back:
            br = f32_branch(O.random_branch(rng, len(snps), [3, 2, 1]))
            branches.append(br)
            ctx.add_branch(snps, br.layer_widths, br.act, br.prior)
        ctx.finalize()
        for b, br in enumerate(branches):
            ctx.set_params(b, O.param_vec(br.weights, br.biases))
        pred = ctx.predict_many(np.arange(len(back)))
        mu, sd = ctx.genotype_stats()
    b = int(np.argmax([len(x) for x in back]))
    X = x_std(g[back[b]], mu[back[b]], sd[back[b]])
    assert norm_rel(pred[b], O.predict(branches[b], X)) < 1e-5
