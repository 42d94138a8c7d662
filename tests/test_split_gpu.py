"""GPU checks of bann.io.split_train_test and bann.io.fill_missing_a2 (scripts/split_train_test.sh and
scripts/fill_missing_a2.sh without PLINK) on tests/golden/plink/small, and on the same fileset with some
of its calls made missing: the written filesets against numpy on the numpy-decoded input."""
import os
import shutil

import numpy as np
import pytest

import subset_reference as S

pytestmark = pytest.mark.gpu

PLINK = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plink")
SIG = b"\x6c\x1b\x01"


def lines_of(path):
    return open(path, "rb").read().splitlines(keepends=True)


@pytest.fixture(params=["golden", "with_missing"])
def fileset(request, tmp_path):
    """(stem, int8 [M][n] genotypes with -1 for missing): the golden fileset, copied so that the outputs
    land in tmp_path; or the same with a sixth of its calls rewritten as missing (01)"""
    from bann.io import encode_bed_payload
    stem = str(tmp_path / "small")
    for ext in (".bed", ".bim", ".fam"):
        shutil.copy(os.path.join(PLINK, "small" + ext), stem + ext)
    n, M = len(lines_of(stem + ".fam")), len(lines_of(stem + ".bim"))
    g = S.decode_bed(open(stem + ".bed", "rb").read(), n, M)
    if request.param == "with_missing":
        g = g.copy()
        g[np.random.default_rng(5).random(g.shape) < 1 / 6] = -1
        g[:, 7] = np.where(g[:, 7] < 0, 0, g[:, 7])           # one individual with every call
        assert (g < 0).sum() > 10
        open(stem + ".bed", "wb").write(SIG + encode_bed_payload(g))
    return stem, g


def reload(stem, keep=True):
    from bann import BannContext
    ctx = BannContext(0)
    if keep:
        ctx.keep_missing()
    ctx.load_bed(stem)
    return ctx


def assert_fileset_is(stem, want):
    """stem.bed holds the cohort want (int8, -1 missing): by its bytes and as the library reloads it"""
    M, n = want.shape
    data = open(stem + ".bed", "rb").read()
    assert data[:3] == SIG and len(data) == 3 + (n + 3) // 4 * M
    assert np.array_equal(S.decode_bed(data, n, M), want)
    with reload(stem) as ctx:
        assert (ctx.n, ctx.num_markers) == (n, M)
        assert np.array_equal(ctx.download_genotypes(np.arange(M)), S.zero_coded(want))
        assert np.array_equal(ctx.missing_counts(), (want < 0).sum(axis=1))


def test_split_train_test(fileset, tmp_path):
    from bann.io import read_phen, split_indices, split_train_test, write_phen
    stem, g = fileset
    M, n = g.shape
    test_n = n // 3
    write_phen(stem + ".phen", np.arange(n, dtype=np.float32))
    fam = lines_of(stem + ".fam")
    train_idx, test_idx = split_train_test(stem, test_n, seed=11, phen=stem + ".phen")
    want = split_indices(n, test_n, 11)
    assert np.array_equal(train_idx, want[0]) and np.array_equal(test_idx, want[1])
    assert test_idx.size == test_n and np.array_equal(np.sort(np.concatenate([train_idx, test_idx])), np.arange(n))
    os.remove(stem + "_test.dims")             # the dims of this one come from the .fam / .bim line counts
    for out, idx in ((stem + "_train", train_idx), (stem + "_test", test_idx)):
        assert lines_of(out + ".fam") == [fam[i] for i in idx]               # the selected lines, file order
        assert open(out + ".bim", "rb").read() == open(stem + ".bim", "rb").read()
        assert_fileset_is(out, S.subset(g, individuals=idx))
        assert np.array_equal(read_phen(out + ".phen"), idx.astype(np.float32))
    assert sorted(lines_of(stem + "_train.fam") + lines_of(stem + "_test.fam")) == sorted(fam)
    assert open(stem + "_train.dims").read() == f"{n - test_n}\t{M}"


def test_split_train_test_named_outputs_without_presence(fileset, tmp_path):
    """out_train / out_test, no .phen, and keep_missing off: a missing call is written as homozygous A2"""
    from bann.io import split_train_test
    stem, g = fileset
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    train_idx, test_idx = split_train_test(stem, 5, seed=2, out_train=a, out_test=b, keep_missing=False)
    assert not os.path.exists(stem + "_train.bed") and not os.path.exists(a + ".phen")
    assert_fileset_is(a, S.zero_coded(S.subset(g, individuals=train_idx)))
    assert_fileset_is(b, S.zero_coded(S.subset(g, individuals=test_idx)))


def test_fill_missing_a2(fileset, tmp_path):
    from bann.io import fill_missing_a2
    stem, g = fileset
    out = str(tmp_path / "filled")
    fill_missing_a2(stem, out)
    for ext in (".fam", ".bim"):
        assert open(out + ext, "rb").read() == open(stem + ext, "rb").read()
    assert_fileset_is(out, S.zero_coded(g))
    with reload(out) as ctx, reload(stem, keep=False) as plain:
        allm = np.arange(g.shape[0])
        assert np.array_equal(ctx.missing_counts(), np.zeros(g.shape[0], np.int32))
        assert np.array_equal(ctx.download_genotypes(allm), plain.download_genotypes(allm))
