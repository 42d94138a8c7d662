"""The linear score from the resident 2-bit image, the linear-model simulator and the simulate-xy
cohorts on the device (kernels_lin.hip, bann_genotypes_synthetic_maf, bann_genotypes_save_bed) against
the numpy restatement of tests/linear_reference.py.

Score shapes: M = 700 markers, entries cut into chunks of 256 (three chunks, the last one ragged:
700 = 256 + 256 + 188, 701 with the overlap), K in {1, 3, 5} (one pass holds 4 columns), and

| n    | exercises                                                            |
| 5    | less than one dword of a row                                         |
| 64   | exactly one 64-individual tile                                       |
| 65   | one individual into the second tile                                  |
| 4097 | one individual past a workgroup's stripe of 4096: two stripes        |
"""
import json
import math
import os

import numpy as np
import pytest

import linear_reference as R

pytestmark = pytest.mark.gpu

M = 700
CHUNK = 256
PLINK = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plink")
UNIFORM = [np.arange(100 * g, 100 * g + 100, dtype=np.int32) for g in range(7)]
# marker 99 sits in groups 0 and 1
OVERLAP = [np.arange(0, 100, dtype=np.int32), np.arange(99, 200, dtype=np.int32)] + UNIFORM[2:]
P_SEED = R.P_SEED


def refused(code, fn, *args, **kw):
    from bann import BannError
    with pytest.raises(BannError) as e:
        fn(*args, **kw)
    assert e.value.code == code, e.value
    return str(e.value)


def norm_rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def random_effects(K, E, seed):
    return np.random.default_rng(seed).normal(size=(K, E)).astype(np.float32)


_COHORTS = {}


def cohort(n):
    """(context with chunks of 256 entries, x_std f64 [n][M]) of the synthetic cohort of n individuals"""
    if n not in _COHORTS:
        from bann import BannContext
        c = BannContext(0)
        c.synthetic_genotypes(n, M, 100 + n)
        c.linear_chunk(CHUNK)
        x = R.standardize(c.download_genotypes(np.arange(M)), *c.genotype_stats())
        _COHORTS[n] = (c, x)
    return _COHORTS[n]


@pytest.mark.parametrize("n", [5, 64, 65, 4097])
@pytest.mark.parametrize("groups", [UNIFORM, OVERLAP], ids=["uniform", "overlap"])
def test_score_against_f64(n, groups):
    c, x = cohort(n)
    E = sum(len(g) for g in groups)
    assert -(-E // CHUNK) == 3 and E % CHUNK != 0
    for K in (1, 3, 5):
        eff = random_effects(K, E, 7 * K + n)
        got = c.linear_score(groups, eff)
        ref = R.score(x, groups, eff)
        assert got.shape == (K, n) and got.dtype == np.float32
        for k in range(K):
            err = norm_rel(got[k], ref[k])
            print(f"n {n} E {E} K {K} column {k}: norm-rel {err:.2e}")
            assert err <= 1e-5
    one = c.linear_score(groups, eff[2])                    # [E] in, [n] out
    assert one.shape == (n,) and np.array_equal(one, got[2])


def test_score_default_chunk_and_timing():
    c, x = cohort(4097)
    eff = random_effects(2, M, 3)
    c.linear_chunk(0)                                       # the default: one chunk at E = 700
    try:
        got = c.linear_score(UNIFORM, eff)
    finally:
        c.linear_chunk(CHUNK)
    assert max(norm_rel(got[k], R.score(x, UNIFORM, eff)[k]) for k in range(2)) <= 1e-5
    assert c.linear_timing() > 0.0
    refused(-5, c.linear_chunk, -1)


def test_score_constant_column_and_field_three():
    from bann import BannContext
    rng = np.random.default_rng(5)
    n, m = 65, 8
    g = rng.integers(0, 3, size=(m, n)).astype(np.int8)
    g[2] = 1                                                # sigma = 0: contributes 0
    g[5] = 3                                                # field value 3, constant
    g[6, ::7] = 3                                           # field value 3 among called values: counts as 3
    with BannContext(0) as c:
        c.upload_genotypes(g)
        mu, sd = c.genotype_stats()
        assert sd[2] == 0 and sd[5] == 0 and sd[6] > 0
        x = R.standardize(c.download_genotypes(np.arange(m)), mu, sd)
        groups = [np.arange(0, 4), np.arange(4, 8)]
        eff = random_effects(2, m, 1)
        got = c.linear_score(groups, eff)
        ref = R.score(x, groups, eff)
        assert max(norm_rel(got[k], ref[k]) for k in range(2)) <= 1e-5
        only = np.zeros(m, np.float32)
        only[2] = only[5] = 1.0
        assert np.all(c.linear_score(groups, only) == 0.0)


def test_score_ignores_keep_missing():
    from bann import BannContext
    from bann.io import read_grouping
    groups = read_grouping(os.path.join(PLINK, "small.gene_grouping"))
    assert 1 in groups[0] and 1 in groups[1]                # marker 1 in two groups
    eff = random_effects(3, sum(len(g) for g in groups), 2)
    out = []
    for keep in (False, True):
        with BannContext(0) as c:
            if keep:
                c.keep_missing()
            c.load_bed(os.path.join(PLINK, "small"))
            out.append(c.linear_score(groups, eff))
            if not keep:
                x = R.standardize(c.download_genotypes(np.arange(c.num_markers)), *c.genotype_stats())
                assert max(norm_rel(out[0][k], R.score(x, groups, eff)[k]) for k in range(3)) <= 1e-5
    assert np.array_equal(out[0], out[1])
    # the fixture has no missing call; a payload that has some, so that a presence image is really kept
    from bann.io import encode_bed_payload
    g = np.random.default_rng(3).integers(-1, 3, size=(14, 67)).astype(np.int8)
    out = []
    for keep in (False, True):
        with BannContext(0) as c:
            if keep:
                c.keep_missing()
            c.upload_bed(encode_bed_payload(g), 67, 14)
            if keep:
                assert np.array_equal(c.missing_counts(), (g < 0).sum(axis=1))
            out.append(c.linear_score(groups, eff))
    assert np.array_equal(out[0], out[1])


def test_score_bits():
    c, _ = cohort(65)
    E = sum(len(g) for g in OVERLAP)
    eff = random_effects(5, E, 11)
    a = c.linear_score(OVERLAP, eff)
    assert np.array_equal(a, c.linear_score(OVERLAP, eff))                 # two calls
    for k in range(5):                                                     # a column alone
        assert np.array_equal(c.linear_score(OVERLAP, eff[k]), a[k]), k
    perm = np.array([3, 0, 4, 2, 1])
    assert np.array_equal(c.linear_score(OVERLAP, eff[perm]), a[perm])     # permuted columns
    assert np.array_equal(c.linear_score(OVERLAP, eff[:2]), a[:2])         # K does not matter


def test_score_after_finalize():
    from bann import BannContext
    eff = random_effects(2, M, 4)
    ref_c, _ = cohort(65)
    want = ref_c.linear_score(UNIFORM, eff)
    for free in (False, True):
        with BannContext(0) as c:
            c.synthetic_genotypes(65, M, 100 + 65)
            c.linear_chunk(CHUNK)
            c.add_branch(np.arange(10, dtype=np.int32), [2, 1])
            c.finalize(free_raw=free)
            if free:
                assert "freed" in refused(-4, c.linear_score, UNIFORM, eff)
            else:
                assert np.array_equal(c.linear_score(UNIFORM, eff), want)


def test_score_refusals():
    from bann import BannContext
    c, _ = cohort(65)
    eff = random_effects(1, M, 1)
    off = np.array([0, 400, 300, 700], np.int64)
    mk = np.arange(M, dtype=np.int32)
    import ctypes as C
    out = np.zeros((1, 65), np.float32)

    def raw(off, mk, K):
        c._check(c._lib.bann_genotypes_linear_score(c._h, len(off) - 1, off.ctypes.data_as(C.POINTER(C.c_int64)),
                                                     mk.ctypes.data_as(C.POINTER(C.c_int32)),
                                                     eff.ctypes.data_as(C.POINTER(C.c_float)), K,
                                                     out.ctypes.data_as(C.POINTER(C.c_float))))
    refused(-5, raw, off, mk, 1)                                           # offsets decrease
    refused(-5, raw, np.array([0, 700], np.int64), mk, 0)                  # K < 1
    bad = mk.copy()
    bad[699] = M
    refused(-5, raw, np.array([0, 700], np.int64), bad, 1)                 # a marker outside the cohort
    with BannContext(0) as empty:
        refused(-4, empty.linear_score, UNIFORM, eff)                      # no cohort


@pytest.fixture(scope="module")
def any_ctx():
    return cohort(65)[0]


@pytest.mark.parametrize("E", [1, 255, 257, 70001])
def test_effects_against_restatement(any_ctx, E):
    """70 001 entries cross every histogram-pass boundary of a 16-bit digit of (key << 32 | index)"""
    c = any_ctx
    h = 0.7
    cases = [dict(num_effective=e) for e in (1, E - 1, E) if e >= 1] + [dict(proportion_effective=0.25), dict()]
    for kw in cases:
        seed = P_SEED if "proportion_effective" in kw else 5
        want, m_want = R.effects(seed, E, h, **kw)
        got, m = c.linear_effects(E, h, seed=seed, **kw)
        assert m == m_want and got.shape == (E,), (kw, m, m_want)
        assert np.array_equal(got != 0, want != 0), kw                     # the mask, exactly
        assert np.all(np.abs(got.astype(np.float64) - want) <= 2.0 ** -23 * np.abs(want)), kw
    refused(-5, c.linear_effects, E, h, num_effective=0)
    refused(-5, c.linear_effects, E, h, num_effective=E + 1)
    # num_effective takes precedence over the proportion
    a, _ = c.linear_effects(E, h, num_effective=1, proportion_effective=0.25, seed=5)
    assert np.array_equal(a, c.linear_effects(E, h, num_effective=1, seed=5)[0])


def test_effects_refusals(any_ctx):
    for h in (0.0, 1.5, -0.1, float("nan")):
        refused(-5, any_ctx.linear_effects, 10, h)
    refused(-5, any_ctx.linear_effects, 0, 0.5)
    assert "no effective marker" in refused(-5, any_ctx.linear_effects, 50, 0.5, proportion_effective=0.0)


def ks_normal(v, sd):
    x = np.sort(v) / (sd * math.sqrt(2.0))
    cdf = 0.5 * (1.0 + np.array([math.erf(t) for t in x]))
    n = v.size
    return max(np.max(np.arange(1, n + 1) / n - cdf), np.max(cdf - np.arange(n) / n))


def test_effects_distribution(any_ctx):
    """179 200 kept draws: the Kolmogorov-Smirnov statistic against N(0, h / m) below 1.95 / sqrt(N), the
    sum of squares within three standard errors (h sqrt(2 / N)) of h"""
    N, h = 179200, 0.5
    got, m = any_ctx.linear_effects(N, h, seed=2000)
    v = got.astype(np.float64)
    assert m == N and np.all(v != 0)
    sd = float(np.sqrt(np.float32(h) / np.float32(N)))
    ks, ss = ks_normal(v, sd), float(np.sum(v * v))
    print(f"KS {ks:.5f} (bound {1.95 / math.sqrt(N):.5f}) sum of squares {ss:.6f} vs {h}")
    assert ks < 1.95 / math.sqrt(N)
    assert abs(ss - h) <= 3.0 * h * math.sqrt(2.0 / N)


def test_simulate_y_columns():
    c, _ = cohort(4097)
    n = 4097
    eff = random_effects(3, M, 21)
    seeds = [5, 6, 7]
    y, g, st = c.linear_simulate_y(UNIFORM, eff, 0.5, seeds, return_g=True)
    assert np.array_equal(g, c.linear_score(UNIFORM, eff))                 # g: the score call's bits
    for k in range(3):
        g64, y64 = g[k].astype(np.float64), y[k].astype(np.float64)
        sg, cg, sy, cy, rv = st[k]["sums"]
        s2 = float(np.var(g64, ddof=1))
        print(f"column {k}: s2 {s2:.6g} rv {rv:.6g} mean y {sy / n:.6g} var y {cy / (n - 1):.6g}")
        assert abs(sg - float(np.sum(g64))) <= 1e-6 * float(np.sum(np.abs(g64)))
        assert abs(cg / (n - 1) - s2) <= 1e-6 * s2
        assert abs(rv - s2) <= 1e-6 * s2                                   # rv = s2 (1 / 0.5 - 1)
        m64, v64 = float(np.mean(y64)), float(np.var(y64, ddof=1))
        assert abs(sy / n - m64) <= 1e-6 * float(np.mean(np.abs(y64))) and abs(cy / (n - 1) - v64) <= 1e-6 * v64
        assert st[k]["mean"] == float(np.float32(sy / n)) and st[k]["env_variance"] == float(np.float32(rv))
        d = y64 - g64                                                      # the noise alone
        assert abs(float(np.mean(d))) <= 5.0 * math.sqrt(rv / n)
        assert abs(float(np.var(d, ddof=1)) - rv) <= 5.0 * math.sqrt(2.0 / (n - 1)) * rv
        y1, st1 = c.linear_simulate_y(UNIFORM, eff[k], 0.5, seeds[k])      # the column alone
        assert np.array_equal(y1, y[k]) and st1 == st[k], k
    assert not np.array_equal(y[0] - g[0], y[1] - g[1])                    # another seed, another noise
    y_q, st_q = c.linear_simulate_y(UNIFORM, eff[0], 0.25, 5)
    assert abs(st_q["sums"][4] - 3.0 * st[0]["sums"][1] / (n - 1)) <= 1e-6 * st_q["sums"][4]


def test_simulate_y_h1_and_refusals():
    from bann import BannContext
    c, _ = cohort(65)
    eff = random_effects(2, M, 8)
    y, g, st = c.linear_simulate_y(UNIFORM, eff, 1.0, [1, 2], return_g=True)
    assert np.array_equal(y, g) and np.array_equal(g, c.linear_score(UNIFORM, eff))
    assert all(s["env_variance"] == 0.0 and s["sums"][4] == 0.0 for s in st)
    for h in (0.0, 1.5):
        refused(-5, c.linear_simulate_y, UNIFORM, eff, h, [1, 2])
    with BannContext(0) as one:
        one.upload_genotypes(np.array([[0], [1], [2]], np.int8))
        refused(-2, one.linear_simulate_y, [np.arange(3)], np.ones(3, np.float32), 0.5, 1)


def test_synthetic_genotypes_with_mafs():
    from bann import BannContext
    n, m = 20000, 64
    mafs = np.linspace(0.05, 0.5, m).astype(np.float32)
    got = []
    for seed in (3, 3, 4):
        with BannContext(0) as c:
            c.synthetic_genotypes(n, m, seed, mafs=mafs)
            got.append((c.download_genotypes(np.arange(m)), *c.genotype_stats()))
    g, mu, sd = got[0]
    assert all(np.array_equal(a, b) for a, b in zip(got[0], got[1]))       # the same seed, the same bits
    assert not np.array_equal(g, got[2][0])                                # the test cohort differs
    assert g.min() >= 0 and g.max() <= 2 and np.all(sd > 0)
    p = mafs.astype(np.float64)
    means = g.astype(np.float64).mean(axis=1)
    assert np.all(np.abs(means - 2.0 * p) <= 5.0 * np.sqrt(2.0 * p * (1.0 - p) / n))
    assert np.allclose(mu, means, rtol=1e-6)
    with BannContext(0) as c:
        refused(-5, c.synthetic_genotypes, 10, 2, 1, mafs=np.array([0.2, 1.5], np.float32))


def test_save_bed_fixture(tmp_path):
    from bann import BannContext
    raw = open(os.path.join(PLINK, "random.bed"), "rb").read()
    assert open(os.path.join(PLINK, "random.dims")).read() == "100\t20"
    with BannContext(0) as c:
        c.load_bed(os.path.join(PLINK, "random"))
        c.save_bed(str(tmp_path / "copy"))
    assert open(tmp_path / "copy.bed", "rb").read() == raw
    assert open(tmp_path / "copy.dims", "rb").read() == open(os.path.join(PLINK, "random.dims"), "rb").read()


def test_save_bed_keeps_missing_calls(tmp_path):
    from bann import BannContext
    state = []
    for stem in (os.path.join(PLINK, "small"), str(tmp_path / "again")):
        with BannContext(0) as c:
            c.keep_missing()
            c.load_bed(stem)
            state.append((c.download_genotypes(np.arange(c.num_markers)), c.missing_counts(), c.n))
            if not state[1:]:
                c.save_bed(str(tmp_path / "again"))
    assert state[0][2] == state[1][2] and np.array_equal(state[0][0], state[1][0])
    assert np.array_equal(state[0][1], state[1][1])


@pytest.mark.parametrize("n", [1, 4, 5, 67])
def test_save_bed_round_trip(tmp_path, n):
    from bann import BannContext
    from bann.io import encode_bed_payload
    rng = np.random.default_rng(n)
    g = rng.integers(-1, 3, size=(9, n)).astype(np.int8)
    g[0, 0] = -1
    payload = encode_bed_payload(g)
    with BannContext(0) as c:
        c.keep_missing()
        c.upload_bed(payload, n, 9)
        c.save_bed(str(tmp_path / "kept"))
    assert open(tmp_path / "kept.bed", "rb").read() == R.bed_file_bytes(g)
    assert open(tmp_path / "kept.dims").read() == f"{n}\t9"
    with BannContext(0) as c:                              # no presence image: a missing call was read as 0
        c.upload_bed(payload, n, 9)
        c.save_bed(str(tmp_path / "plain"))
    assert open(tmp_path / "plain.bed", "rb").read() == R.bed_file_bytes(np.where(g < 0, 0, g))


def test_save_bed_refuses_field_three(tmp_path):
    from bann import BannContext
    with BannContext(0) as c:
        c.upload_genotypes(np.array([[0, 1, 2, 3, 1]], np.int8))
        refused(-5, c.save_bed, str(tmp_path / "bad"))
    assert not os.path.exists(tmp_path / "bad.bed")


LINEAR_FILES = ["args.json", "model.params", "test.phen", "test_phen_stats.json", "train.phen", "train_phen_stats.json"]
JSON_FILES = ["genetic_values_test.json", "genetic_values_train.json", "phen_test.json", "phen_train.json"]
XY_FILES = ["test.bed", "test.dims", "test.groups", "train.bed", "train.dims", "train.groups"]


def test_simulate_y_linear_files(tmp_path):
    from bann import BannContext, simulate
    from bann.io import read_grouping, read_phen
    stem, groups = os.path.join(PLINK, "small"), os.path.join(PLINK, "small.gene_grouping")
    path = simulate.simulate_y_linear(stem, stem, groups, str(tmp_path), heritability=0.5, num_effective=3, seed=4,
                                      json_data=True)
    assert path == str(tmp_path / "Linear_h0.5_me3_rep1")
    assert sorted(os.listdir(path)) == sorted(LINEAR_FILES + JSON_FILES)
    text = open(os.path.join(path, "model.params")).read()
    lm = json.loads(text)
    gl = read_grouping(groups)
    assert text.endswith("}\n") and list(lm) == ["num_branches", "num_markers_per_branch", "effects"]
    assert lm["num_branches"] == 3 and lm["num_markers_per_branch"] == [len(g) for g in gl] == [4, 4, 6]
    eff = np.concatenate([np.asarray(e, np.float32) for e in lm["effects"]])
    assert int(np.count_nonzero(eff)) == 3
    assert text == R.linear_model_line(gl, eff)
    args = json.load(open(os.path.join(path, "args.json")))
    assert args["model_type"] == "Linear" and args["num_effective"] == 3 and args["seed"] == 4 and args["json_data"]
    with BannContext(0) as c:                              # model.params reproduces g through linear_score
        c.load_bed(stem)
        g = c.linear_score(gl, eff)
    g_train = np.asarray(json.load(open(os.path.join(path, "genetic_values_train.json")))["y"], np.float32)
    assert np.array_equal(g, g_train)
    y_train = read_phen(os.path.join(path, "train.phen"))
    assert np.array_equal(np.asarray(json.load(open(os.path.join(path, "phen_train.json")))["y"], np.float32), y_train)
    assert not np.array_equal(y_train, read_phen(os.path.join(path, "test.phen")))   # another noise seed
    st = json.load(open(os.path.join(path, "train_phen_stats.json")))
    assert st["env_variance"] > 0 and abs(st["mean"] - float(np.mean(y_train, dtype=np.float64))) <= 1e-6
    plain = simulate.simulate_y_linear(stem, stem, groups, str(tmp_path), heritability=1.0, proportion_effective=0.5,
                                       seed=P_SEED)
    assert os.path.basename(plain) == "Linear_h1_pe0.5_rep1" and sorted(os.listdir(plain)) == LINEAR_FILES


def test_simulate_y_linear_replicates(tmp_path):
    from bann import simulate
    stem, groups = os.path.join(PLINK, "small"), os.path.join(PLINK, "small.gene_grouping")
    kw = dict(heritability=0.5, json_data=True)
    many = simulate.simulate_y_linear(stem, stem, groups, str(tmp_path), seed=9, replicates=3, **kw)
    assert [os.path.basename(p) for p in many] == [f"Linear_h0.5_rep{i}" for i in (1, 2, 3)]
    for r, p in enumerate(many):
        single = simulate.simulate_y_linear(stem, stem, groups, str(tmp_path), seed=9 + 2 * r, **kw)
        assert os.path.basename(single) == f"Linear_h0.5_rep{4 + r}"
        assert sorted(os.listdir(single)) == sorted(os.listdir(p)) == sorted(LINEAR_FILES + JSON_FILES)
        for f in os.listdir(p):
            assert open(os.path.join(p, f), "rb").read() == open(os.path.join(single, f), "rb").read(), (r, f)
    assert open(os.path.join(many[0], "train.phen"), "rb").read() != open(os.path.join(many[1], "train.phen"), "rb").read()


def test_simulate_y_json_data_opt_in(tmp_path):
    from bann import simulate
    stem, groups = os.path.join(PLINK, "small"), os.path.join(PLINK, "small.gene_grouping")
    a = simulate.simulate_y(stem, stem, groups, "ridge_ard", "tanh", 1, str(tmp_path / "a"), heritability=0.5, seed=4)
    b = simulate.simulate_y(stem, stem, groups, "ridge_ard", "tanh", 1, str(tmp_path / "b"), heritability=0.5, seed=4,
                            json_data=True)
    assert sorted(set(os.listdir(b)) - set(os.listdir(a))) == JSON_FILES and len(os.listdir(a)) == 7
    for f in ("train.phen", "test.phen", "model.params", "model.bin", "train_phen_stats.json"):
        assert open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read(), f
    from bann.io import read_phen
    y = np.asarray(json.load(open(os.path.join(b, "phen_test.json")))["y"], np.float32)
    assert np.array_equal(y, read_phen(os.path.join(b, "test.phen")))


def test_simulate_xy_linear(tmp_path):
    from bann import BannContext, simulate
    from bann.io import read_grouping
    path = simulate.simulate_xy("linear", None, 3, 33, 65, 4, None, 1, str(tmp_path), heritability=0.5,
                                proportion_effective=0.5, seed=P_SEED)
    assert path == str(tmp_path / "Linear_b3_wh4_ws4_d1_m33_n65_h0.5_pe0.5_rep1")
    assert sorted(os.listdir(path)) == sorted(LINEAR_FILES + XY_FILES)
    assert open(os.path.join(path, "train.dims")).read() == "65\t99"
    gl = read_grouping(os.path.join(path, "test.groups"))
    assert [g.tolist() for g in gl] == [list(range(33 * b, 33 * b + 33)) for b in range(3)]
    lm = json.loads(open(os.path.join(path, "model.params")).read())
    assert lm["num_markers_per_branch"] == [33, 33, 33]
    geno = []
    for stem in ("train", "test"):
        with BannContext(0) as c:
            c.load_bed(os.path.join(path, stem))
            assert (c.n, c.num_markers) == (65, 99)
            geno.append(c.download_genotypes(np.arange(99)))
    assert not np.array_equal(geno[0], geno[1])            # the same frequencies, another seed


def test_simulate_xy_network_trains(tmp_path):
    from bann import MCMCConfig, simulate
    from bann.io import read_phen
    path = simulate.simulate_xy("ridge_ard", "tanh", 3, 33, 65, 4, 2, 1, str(tmp_path), heritability=0.5,
                                init_param_variance=1.0, seed=3)
    assert path == str(tmp_path / "RidgeARD_Tanh_b3_wh4_ws2_d1_m33_n65_h0.5_v1.0_rep1")
    assert sorted(os.listdir(path)) == sorted(LINEAR_FILES + XY_FILES + ["model.bin"])
    cfgs = json.loads(open(os.path.join(path, "model.params")).read())
    assert [b["num_markers"] for b in cfgs] == [33, 33, 33] and cfgs[0]["layer_widths"] == [4, 2, 1]
    st = json.load(open(os.path.join(path, "train_phen_stats.json")))
    assert st["env_variance"] >= 0.01
    y = read_phen(os.path.join(path, "train.phen"))
    assert y.shape == (65,)
    net = simulate.new_net(os.path.join(path, "train"), os.path.join(path, "train.groups"), "ridge_ard", "tanh", 1,
                           seed=3)
    cfg = MCMCConfig(hmc_integration_length=5, chain_length=1, burn_in=0, hmc_step_size_factor=0.1)
    net.train_network(y, cfg, outdir=str(tmp_path / "network"))
    assert np.all(np.isfinite(net.predict()))
    c = net._ctx
    net.close()
    c.close()


def teardown_module(module):
    for c, _ in _COHORTS.values():
        c.close()
    _COHORTS.clear()
