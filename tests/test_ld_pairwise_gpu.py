"""GPU checks of the pairwise-complete LD (the presence image of kernels_data.hip, the six bands of
kernels_ld.hip, bann_ld.hip): the f32 band is bit-equal to tests/ld_pairwise_reference.py and N equal
as int32, the graph equals its edge set, and group-by-ld on a cohort with 15 % missing calls finds the
groups of the complete data.  Every cohort is built in numpy with its missing calls (-1), encoded to a
.bed payload by the reference's own encoder and loaded with keep_missing + upload_bed (load_bed where
a test says so).  The contexts hold genotypes only unless a test says otherwise."""
import os

import numpy as np
import pytest

import ld_pairwise_reference as P
import ld_reference as R

pytestmark = pytest.mark.gpu

E_STATE, E_ARG = -4, -5


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


def assert_pairs_equal(got, want):
    assert got.shape == want.shape and got.dtype == np.int32
    bad = np.argwhere(got != want)
    assert bad.size == 0, (len(bad), bad[:5].tolist(), [(got[tuple(b)], want[tuple(b)]) for b in bad[:5]])


def context(Ctx, name, keep=True):
    ctx = Ctx(0)
    if keep:
        ctx.keep_missing()
    if name in ("small", "random"):
        ctx.load_bed(os.path.join(P.PLINK, name))
    else:
        gm = P.cohort(name)
        ctx.upload_bed(P.encode_bed(gm), gm.shape[1], gm.shape[0])
    return ctx


def graph_edges(ctx, *args, **kw):
    off, nb = ctx.ld_graph(*args, **kw)
    assert off.dtype == np.int64 and nb.dtype == np.int32 and off[0] == 0 and off[-1] == nb.size
    return R.csr_edges(off, nb)


@pytest.mark.parametrize("name,window", [("small", 10), ("random", 25), ("blocks", 137), ("deep", 69)])
def test_band_and_pairs_bit_equal(Ctx, name, window):
    gm = P.cohort(name)
    M = gm.shape[0]
    want, want_n = P.ref_band(name, window), P.ref_npairs(name, window)
    with context(Ctx, name) as ctx:
        got, got_n = ctx.ld_band(window, pairwise=True, return_pairs=True)
        assert ctx.ld_timing() > 0.0
        assert_band_equal(got, want)
        assert_pairs_equal(got_n, want_n)
        assert_band_equal(ctx.ld_band(window, pairwise=True), want)          # without the N output
        if name == "blocks":
            # marker 17 has no call at all: its row and its column are r2 0 with N 0
            assert np.all(got[17] == 0) and np.all(got_n[17] == 0)
            for j in range(max(0, 17 - window), 17):
                assert got[j, 17 - j - 1] == 0 and got_n[j, 17 - j - 1] == 0
            assert len(P.edges(gm, window, 0.5)) >= 1000
            # chunks, as test_band_chunked_retrieval
            parts = [ctx.ld_band(window, f, min(7, M - f), pairwise=True, return_pairs=True) for f in range(0, M, 7)]
            assert_band_equal(np.concatenate([p[0] for p in parts]), want)
            assert_pairs_equal(np.concatenate([p[1] for p in parts]), want_n)
            for f in (0, 1, 63, 64, 127, 128, 200, M - 1):  # chunk size 1, at and around the tile edges
                r, npr = ctx.ld_band(window, f, 1, pairwise=True, return_pairs=True)
                assert_band_equal(r, want[f:f + 1])
                assert_pairs_equal(npr, want_n[f:f + 1])
            assert ctx.ld_band(window, M, 0, pairwise=True).shape == (0, window)
        if name == "deep":
            # 40 is constant among (40, 41)'s present individuals: 0; it varies among (40, 42)'s
            assert got[40, 0] == 0 and got_n[40, 0] > 0 and got[40, 1] > 0
            assert np.all(got[30] == 0) and np.all(got_n[30, :M - 31] > 0)   # zero variance, though present


def test_load_bed_from_a_written_file(Ctx, tmp_path):
    """the file path fills the same presence image as the payload path"""
    gm = P.cohort("blocks")
    M, n = gm.shape
    stem = str(tmp_path / "cohort")
    with open(stem + ".bed", "wb") as f:
        f.write(b"\x6c\x1b\x01" + P.encode_bed(gm))
    with open(stem + ".dims", "w") as f:
        f.write(f"{n} {M}\n")
    with Ctx(0) as ctx:
        ctx.keep_missing()
        ctx.load_bed(stem)
        got, got_n = ctx.ld_band(137, pairwise=True, return_pairs=True)
        assert_band_equal(got, P.ref_band("blocks", 137))
        assert_pairs_equal(got_n, P.ref_npairs("blocks", 137))
        assert np.array_equal(ctx.missing_counts(), (gm < 0).sum(axis=1))


def test_missing_counts(Ctx):
    gm = P.cohort("blocks")
    M, n = gm.shape
    want = (gm < 0).sum(axis=1).astype(np.int32)
    assert want[17] == n == 193 and want.min() >= 1   # individual 5 is missing everywhere
    with context(Ctx, "blocks") as ctx:
        got = ctx.missing_counts()
        assert got.dtype == np.int32 and np.array_equal(got, want)
        assert np.array_equal(ctx.missing_counts(130, 45), want[130:175])
        assert ctx.missing_counts(M, 0).size == 0
        from bann import BannError
        with pytest.raises(BannError) as e:
            ctx.missing_counts(M - 1, 2)
        assert e.value.code == E_ARG


def test_padding_is_absent(Ctx):
    """n = 193: three padding codes 00 (a called 2 in a .bed) beside the last individual, 63 padding
    individuals in the last tile: none of them counts"""
    gm = P.cohort("blocks")
    M, n = gm.shape
    with context(Ctx, "blocks") as ctx:
        _, got_n = ctx.ld_band(137, pairwise=True, return_pairs=True)
    assert got_n.max() <= n
    rng = np.random.default_rng(21)
    for _ in range(20):
        j = int(rng.integers(0, M - 1))
        k = int(rng.integers(j + 1, min(M, j + 138)))
        assert got_n[j, k - j - 1] == n - int(((gm[j] < 0) | (gm[k] < 0)).sum()), (j, k)


def test_graph_equals_edge_set(Ctx):
    gm = P.cohort("blocks")
    M = gm.shape[0]
    chrom = (np.arange(M) >= 104).astype(np.int32)   # marker 104 is inside the block 99 .. 108
    bp = (1000 * np.arange(M)).astype(np.int64)
    with context(Ctx, "blocks") as ctx:
        want = P.edges(gm, 137, 0.5)
        assert len(want) >= 1000
        assert graph_edges(ctx, 137, 0.5, pairwise=True) == want
        for max_bp in (0, 4500):
            filt = P.edges(gm, 137, 0.5, chrom, bp, max_bp)
            assert 0 < len(filt) < len(want)
            assert graph_edges(ctx, 137, 0.5, chrom=chrom, bp=bp, max_bp=max_bp, pairwise=True) == filt


def test_graph_threshold_tie_on_duplicates(Ctx):
    """r2_min = 1.0: markers 203, 205, 206 carry the same genotypes with different missing patterns.
    Over a pair's jointly present individuals a = b and qa = qb, so cov^2 = v_a v_b as integers and
    r2 is exactly 1: the reference gives {(203, 205), (203, 206), (205, 206)}, and nothing on the
    zero-coded cohort, where the differing missing calls break the equality."""
    gm = P.cohort("blocks_dups")
    want = P.edges(gm, 137, 1.0)
    assert want == {(203, 205), (203, 206), (205, 206)}
    assert R.edges(P.zero_coded(gm), 137, 1.0) == set()
    with context(Ctx, "blocks_dups") as ctx:
        assert graph_edges(ctx, 137, 1.0, pairwise=True) == want
        assert graph_edges(ctx, 137, 1.0) == set()


def test_results_do_not_depend_on_the_marker_blocks(Ctx):
    """a limit that holds 128 rows of six bands of a 137-marker window: the 300 markers go in three blocks"""
    from bann import BannError
    gm = P.cohort("blocks")
    M, window = gm.shape[0], 137
    want, want_n = P.ref_band("blocks", window), P.ref_npairs("blocks", window)
    with context(Ctx, "blocks") as ctx:
        ctx.ld_scratch_limit(128 * window * 4 * 6)
        got, got_n = ctx.ld_band(window, pairwise=True, return_pairs=True)
        assert_band_equal(got, want)
        assert_pairs_equal(got_n, want_n)
        got, got_n = ctx.ld_band(window, 100, 200, pairwise=True, return_pairs=True)   # blocks 100..227, 228..299
        assert_band_equal(got, want[100:300])
        assert_pairs_equal(got_n, want_n[100:300])
        assert graph_edges(ctx, window, 0.5, pairwise=True) == P.edges(gm, window, 0.5)
        ctx.ld_scratch_limit(128 * window * 4 * 6 - 1)     # one byte short of 128 rows of six bands
        for call in (lambda: ctx.ld_band(window, pairwise=True), lambda: ctx.ld_graph(window, 0.5, pairwise=True)):
            with pytest.raises(BannError) as e:
                call()
            assert e.value.code == E_ARG
        ctx.ld_band(window)                                # the one-band call still fits
        ctx.ld_scratch_limit(0)
        assert_band_equal(ctx.ld_band(window, pairwise=True), want)


def test_no_missing_calls(Ctx):
    """keep on, a cohort without a missing call: the pairwise band is ld_band's, N is n inside the band"""
    g = P.complete("blocks")
    M, n = g.shape
    with Ctx(0) as ctx:
        ctx.keep_missing()
        ctx.upload_bed(P.encode_bed(g), n, M)
        assert np.all(ctx.missing_counts() == 0)
        plain = ctx.ld_band(137)
        assert_band_equal(plain, R.band(g, 137))
        got, got_n = ctx.ld_band(137, pairwise=True, return_pairs=True)
        assert_band_equal(got, plain)
        inside = np.add.outer(np.arange(M), np.arange(1, 138)) < M
        assert_pairs_equal(got_n, np.where(inside, n, 0).astype(np.int32))
        assert graph_edges(ctx, 137, 0.5, pairwise=True) == R.edges(g, 137, 0.5)
    with Ctx(0) as ctx:   # int8 upload: everyone is present
        ctx.keep_missing()
        ctx.upload_genotypes(g)
        assert np.all(ctx.missing_counts() == 0)
        assert_band_equal(ctx.ld_band(137, pairwise=True), plain)


def test_existing_behaviour_untouched(Ctx):
    """keep on and missing calls present: ld_band, ld_graph and the genotype image are the zero-coded ones"""
    gm = P.cohort("blocks")
    z = P.zero_coded(gm)
    with context(Ctx, "blocks") as ctx:
        assert_band_equal(ctx.ld_band(137), R.band(z, 137))
        assert graph_edges(ctx, 137, 0.5) == R.edges(z, 137, 0.5)
        assert np.array_equal(ctx.download_genotypes(np.arange(z.shape[0])), z)
        mu_keep, sd_keep = ctx.genotype_stats()
    with context(Ctx, "blocks", keep=False) as ctx:
        mu, sd = ctx.genotype_stats()
        assert np.array_equal(bits(mu), bits(mu_keep)) and np.array_equal(bits(sd), bits(sd_keep))
        assert np.array_equal(ctx.download_genotypes(np.arange(z.shape[0])), z)


def test_state_errors(Ctx):
    from bann import BannError
    gm = P.cohort("groups")
    payload = P.encode_bed(gm)
    M, n = gm.shape
    snps = np.arange(9, dtype=np.int32)

    def refused(ctx, code):
        for call in (lambda: ctx.ld_band(40, pairwise=True), lambda: ctx.ld_graph(40, 0.5, pairwise=True),
                     lambda: ctx.missing_counts()):
            with pytest.raises(BannError) as e:
                call()
            assert e.value.code == code

    with Ctx(0) as ctx:   # keep off
        ctx.upload_bed(payload, n, M)
        refused(ctx, E_STATE)
        with pytest.raises(BannError) as e:   # after a load
            ctx.keep_missing()
        assert e.value.code == E_STATE
        ctx.ld_band(40)
    with Ctx(0) as ctx:   # keep on, before any genotypes
        ctx.keep_missing()
        refused(ctx, E_STATE)
        ctx.upload_bed(payload, n, M)
        for w in (0, -3):
            with pytest.raises(BannError) as e:
                ctx.ld_band(w, pairwise=True)
            assert e.value.code == E_ARG
        ctx.add_branch(snps, [2, 1, 1])
        ctx.finalize(free_raw=False)
        assert_band_equal(ctx.ld_band(40, pairwise=True), P.ref_band("groups", 40))
    with Ctx(0) as ctx:   # the images freed at finalize
        ctx.keep_missing()
        ctx.upload_bed(payload, n, M)
        ctx.add_branch(snps, [2, 1, 1])
        ctx.finalize(free_raw=True)
        refused(ctx, E_STATE)


def test_group_by_ld_end_to_end(Ctx):
    """15 % missing calls: the pairwise grouping is the complete data's (6 groups, nobody left over), the
    zero-coded one has fallen apart (no group, all 57 markers left over)"""
    from bann.io import encode_bed_payload, group_by_ld
    gm = P.cohort("groups")
    M, n = gm.shape
    want, want_un = R.centered(R.adjacency(M, P.edges(gm, 40, 0.5)), 1)
    assert len(want) == 6 and want_un == 0
    full, full_un = R.centered(R.adjacency(M, R.edges(P.complete("groups"), 40, 0.5)), 1)
    assert len(full) == 6 and full_un == 0
    with Ctx(0) as ctx:
        ctx.keep_missing()
        ctx.upload_bed(encode_bed_payload(gm), n, M)
        groups, ungrouped = group_by_ld(ctx, 40, 0.5, 1, missing="pairwise")
        assert [x.tolist() for x in groups] == want and ungrouped == 0
        groups, ungrouped = group_by_ld(ctx, 40, 0.5, 1, missing="zero")
        assert len(groups) == 0 and ungrouped == 57
        groups, ungrouped = group_by_ld(ctx, 40, 0.5, 1)   # the default is "zero"
        assert len(groups) == 0 and ungrouped == 57
