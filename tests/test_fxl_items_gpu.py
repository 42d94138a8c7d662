"""k_fused_grad_fxl (kernels_fxl.hip) and the head-wave kernel k_fused_grad_fxh (kernels_fxh.hip) on work
items of many tiles, with the delta0 scale set and grown inside an item and with coherent backward digit
sums, against the float64 oracle; the coherent sums on k_fused_grad_fx too; and genotype code 3.

Long items.  An fxl group's split count comes from best_splits alone, so a branch by itself gets one tile per
item at any n the suite can afford.  The item length grows with the branch count instead: 64 same-shape
branches over one shared marker set at n = 3000 (47 tiles, the last one of 56 individuals), contexts built
with BANN_SOLO=0, on a device of 256 compute units:
  chunks        kernel              splits   tiles per item   layers, activation
  10 (m = 577)  fxl, 3 waves        8        5-6              2, tanh
  18 (m = 1100) fxh, 5 waves        4        11-12            3, relu
  32 (m = 2048) fxh, 8 waves        4        11-12            4, tanh
  33 (m = 2100) fxl, 8-chunk waves  4        11-12            3 ([4, 3, 1]), relu
and the two fxh shapes again with BANN_FXL_HEAD=0, where fxl takes them.  Every item is longer than fxh's four
genotype slots, so its slot refill runs.  No GPU test can see a split count: tests/finalize_layout_check.cpp
pins these on the CPU, with the one-branch context's one tile per item.

Targets are drawn independently of the model (tests/test_fx_combine_gpu.py's docstring says why), standard
normal (part 1) or standard normal times 2^(10 ((i // 64) % 3)) (part 2): any three consecutive tiles hold
a growth of the delta0 scale by 2^10 and a second one, so every item of five or more tiles rescales the
digit sums it has twice, wherever it starts.  The designed case of part 2 leaves column 2's scale unset in an
item's first tile while the others are set: ReLU, mu = 0 and sigma = 1, marker m // 2 equal to 2 in the tiles
with (i // 64) % 3 == 0 and to 0 elsewhere, W0[m // 2, 2] = -8 and b0[2] = 1, so in those tiles column 2's
pre-activation is below -10 and its delta0 exactly 0.

Coherent backward sums (part 3).  Identity activation, widths [4, 1], W0 = 0, b0 = 0, mu = 0, sigma = 1,
W1 = signed powers of two: the prediction is exactly 0, the residual is -y and delta0[:, k] = -y W1[k] without
rounding.  A column's digits are V = rint(|delta0| 2^(153 - R)) with R = E + 2 and E the largest biased
exponent the item's column has seen, which puts the largest |delta0| into [2^24, 2^25): a float32 there is
even, so a V with three low digits of 127 needs a larger |delta0| beside it.  With |y| = r = 0x7F7F7F 2^-23
= 0.99607... in K-group 0 (individuals 0 mod 4) and 4 r at one individual of K-group 1 in every tile, the
scale is set by 4 r in every tile of every item and V(r) = 0x7F7F7F = 127 + 127 2^8 + 127 2^16: K-group 0's
three low digits at their largest, the top one 0.  The other individuals have |y| uniform in [r / 2, r)
(K-groups 1 and 2 take rint(V / 4) and rint(V / 16), K-group 3 rint(V / 64) in fx and fxh, field 3 in
place, or V in fxl, field 3 decoded).  All y have one sign, so every digit sum grows linearly: at fx's one
item of 64 tiles per wave (m = 512, n = 16 384, BANN_TARGET_ITEMS=1) they pass 2^24.
Genotypes: (a) all 2; (b) 2 except 0 at individuals 3 mod 4, where field 3's stored -1 and its correction
cancel against a true contribution of zero; (c) the complement of (b).  Each with both signs of y.

Code 3 (part 4).  bann_genotypes_upload accepts the 2-bit value 3, and the statistics, the linear scores, the
LD entries, forward_feed, wx and gx count it as 3.0.  The fx / fxl / fxh tile images store field 3 (individuals
3 mod 4) as code - 1 in two bits, which cannot hold a 3: it reads back as -1.  Measured on an MI355X before the
refusal existed, on this file's cohort whose only 3s sit at individuals 3 mod 4: prediction norm-relative
4.0e-1 (fx), 9.5e-1 (fxl), 5.1e-1 (fxh), gradient 5.8e-2, 3.0e-2, 1.5e-3, with wx and gx at 2.0e-7 and below
(3s anywhere: 3.4e-1, 8.0e-1, 4.4e-1).  bann_finalize now refuses a cohort that holds a 3 for any branch
classified fx or fxl (BANN_E_ARG); the test asserts the refusal and keeps the parity of wx and gx.

Branches.  O.random_branch draws every layer at variance 1 / m; fan_in_branch and off_the_kink below say
how and why the branches here differ: later layers at variance 1 / fan-in, ReLU branches redrawn until no
pre-activation is within 1e-5 of 0.  Both came out of the reference sanity check, not out of a kernel's
results, except that the kink was first met on the device: one unit at -1.75e-7 in a tile of 2^10 targets
put k_fused_grad_fxl at 1.12e-5 where the head-wave kernel, on the same branch, stayed on the oracle's side.

Reference sanity.  The oracle's formulas evaluated in plain numpy float32 on the same inputs (every branch
of every case, on the CPU) against the float64 oracle, worst gradient / prediction / rss error:
  part 1    6.4e-7 / 7.7e-7 / 1.8e-7        part 2    9.5e-7 / 7.7e-7 / 1.1e-7
  designed  6.0e-7 / 8.0e-7 / 1.1e-7        part 3    (b) 7.9e-7, (c) 4.7e-7 (fx 8.9e-7, 7.9e-7); rss 1.0e-7
all below a tenth of the bounds, which are the parity suite's (norm-relative 1e-5 on gradients and predictions,
rss 1e-5 relative).  Part 3's pattern (a) is not: 1.5e-6 (fx 1.3e-6).  There every marker's gradient is the
same sum of n same-sign terms, which float32 adds with a relative error of about 2^-24 sqrt(n / 3) in
sequence whatever the values are, and the case fixes n and the sign; drawing the residuals outside K-group 0
at random in [r / 2, r) instead of at r took it down from 6.0e-6.  The kernels add these in int32, exactly.

Measured on an MI355X (256 compute units), worst gradient error over a part's cases and branches:
  part 1    fxl 4.3e-7   fxh 1.2e-6        part 2    fxl 1.8e-6   fxh 6.2e-6
  designed  fxl 1.4e-6   fxh 5.2e-6        part 3    fx 8.0e-8    fxl 1.6e-7   fxh 2.9e-7
predictions 4.9e-7 at most (designed 1.6e-6), rss 5.3e-8.  fxh, like fx, keeps field 3 in place and takes
K-group 3's digits at 1 / 64 of the column's scale, fxl decodes the field and takes them at the full scale,
which is consistent with fxh's larger figures where the data term carries the gradient (part 2).  Part 1's
alone-against-packed comparison came out bit for bit.  With the digit-sum rescale skipped in a scratch build
(the shr_digits shift of kernels_fxl.hip, of kernels_fxh.hip) every part 2 test of that kernel fails at 0.8
to 2.3 and every test of the other kernel passes; part 1's tanh shapes pass too, its ReLU shapes do not (a
column active for few individuals of an item's first tile grows its scale later even under standard-normal
targets, somewhere among 64 branches).
"""
import numpy as np
import pytest

import bann_oracle as O
from helpers import build_context, f32_branch, norm_rel, x_std

pytestmark = pytest.mark.gpu

TOL = 1e-5
N = 3000
NB = 64
# name: markers, widths, activation, BANN_FXL_HEAD
SHAPES = {
    "fxl-10": (577, [4, 1], "tanh", "1"),
    "fxh-18": (1100, [4, 4, 1], "relu", "1"),
    "fxh-32": (2048, [4, 4, 4, 1], "tanh", "1"),
    "fxl-33": (2100, [4, 3, 1], "relu", "1"),
    "fxl-18": (1100, [4, 4, 1], "relu", "0"),
    "fxl-32": (2048, [4, 4, 4, 1], "tanh", "0"),
}
R127 = float(0x7F7F7F) * 2.0 ** -23  # part 3's |y|: the module docstring derives it
PATTERNS = ("all2", "zero_at_3mod4", "two_at_3mod4")
_cache = {}


@pytest.fixture(scope="module")
def Ctx():
    from bann import BannContext
    return BannContext


def scalar_close(a, b, tol=TOL):
    return abs(a - b) <= tol * max(1.0, abs(b))


def long_item_env(monkeypatch, head):
    monkeypatch.setenv("BANN_SOLO", "0")
    monkeypatch.setenv("BANN_FXL_HEAD", head)


def tile_scale(n):
    return 2.0 ** (10 * ((np.arange(n) // 64) % 3))


def fan_in_branch(rng, m, widths, act):
    """O.random_branch draws every layer at variance 1 / m, which at m = 2048 leaves the hidden activations
    almost constant and the output a cancellation of them: ill-conditioned in any float32.  Here the layers
    after the first have variance 1 / fan-in (their precisions rescaled to match)"""
    br = O.random_branch(rng, m, widths, prior="ridge_ard", act=act)
    for l in range(1, len(widths)):
        s2 = m / float(widths[l - 1])
        br.weights[l] = br.weights[l] * np.sqrt(s2)
        br.weight_precisions[l] = br.weight_precisions[l] / s2
    return br


KINK = 1e-5


def off_the_kink(br, X):
    """ReLU's derivative jumps at 0, and so does the gradient as a function of a pre-activation: a unit within
    float32 rounding of 0 (a few 1e-7 here) may fall on either side of it in the kernel and in the oracle, and
    one such individual in a tile of large targets moves the gradient by 1e-5 and more.  With 64 branches of
    3000 x 8 units about every third case holds one.  A ReLU branch is therefore drawn again until every
    hidden pre-activation of every individual is at least KINK away from 0 (about one draw in five) -- and
    until its prediction is nonzero for half the individuals at least: the norm of a nearly dead network's
    prediction rests on a few small pre-activations, which float32 resolves to 1e-6 only"""
    if br.act != "relu":
        return True
    pre, acts = O.forward_feed(br, X)
    return min(float(np.min(np.abs(p))) for p in pre) >= KINK and float(np.mean(acts[-1] != 0.0)) >= 0.5


def draw_until(ok, draw):
    while True:
        br = draw()
        if ok(br):
            return br


def shape_case(name):
    """genotypes and the 64 branches of a shape, drawn once; the BANN_FXL_HEAD=0 twin of an fxh shape shares them"""
    m, widths, act, _ = SHAPES[name]
    key = ("shape", m)
    if key not in _cache:
        rng = np.random.default_rng(9000 + m)
        g = O.synthetic_genotypes(rng, N, m)
        mu, sd = O.bed_col_stats(g)  # the device's own constants differ in their last bit: far inside KINK
        X = x_std(g, mu.astype(np.float32), sd.astype(np.float32))
        brs = [draw_until(lambda br: off_the_kink(br, X), lambda: f32_branch(fan_in_branch(rng, m, widths, act)))
               for _ in range(NB)]
        _cache[key] = (g, brs)
    return _cache[key]


def designed_case(name):
    """part 2's designed case of a shape (the module docstring), three layers at every shape: parts 1 and 2
    vary the depth"""
    m, widths = SHAPES[name][0], [4, 4, 1]
    key = ("designed", m)
    if key not in _cache:
        rng = np.random.default_rng(9500 + m)
        g = O.synthetic_genotypes(rng, N, m)
        g[m // 2] = np.where((np.arange(N) // 64) % 3 == 0, 2, 0)
        X = g.T.astype(np.float64)

        def draw():
            br = fan_in_branch(rng, m, widths, "relu")
            br.weights[0][m // 2, 2] = -8.0
            br.biases[0][2] = 1.0
            return f32_branch(br)

        brs = [draw_until(lambda br: off_the_kink(br, X), draw) for _ in range(NB)]
        _cache[key] = (g, brs)
    return _cache[key]


def coherent_case(m, n, nb, pattern):
    """part 3: genotypes of a pattern and nb branches whose delta0 is -y W1 exactly"""
    at3 = np.arange(n) % 4 == 3
    row = {"all2": np.full(n, 2), "zero_at_3mod4": np.where(at3, 0, 2), "two_at_3mod4": np.where(at3, 2, 0)}[pattern]
    g = np.tile(row.astype(np.int8)[None, :], (m, 1))
    rng = np.random.default_rng(9700 + m)
    brs = []
    for b in range(nb):
        br = O.random_branch(rng, m, [4, 1], prior="ridge_ard", act="identity")
        br.weights[0][:] = 0.0
        br.biases[0][:] = 0.0
        br.weights[1] = np.array([[1.0], [-(2.0 ** -(b % 4))], [2.0 ** (b % 3)], [-0.5]])
        brs.append(f32_branch(br))
    return g, brs


def coherent_targets(n, nb, sign):
    """|y| = R127 in K-group 0, 4 R127 at one individual of K-group 1 in every tile (its place varies with
    the branch) and uniform in [R127 / 2, R127) elsewhere, all of one sign"""
    rng = np.random.default_rng(9800 + n)
    i = np.arange(n)
    ys = []
    for b in range(nb):
        y = (R127 * rng.uniform(0.5, 1.0, size=n)).astype(np.float32).astype(np.float64)
        y[i % 4 == 0] = R127
        y[i % 64 == (4 * b + 1) % 64] = 4.0 * R127
        ys.append(sign * y)
    return ys


def reference(brs, X, ys):
    """the float64 oracle per branch: predictions, gradient, rss"""
    ref = []
    for br, y in zip(brs, ys):
        gw, gb, rss = O.log_density_gradient(br, X, y)
        ref.append(dict(f=O.predict(br, X), grad=O.param_vec(gw, gb), rss=rss))
    return ref


def f32_targets(rng, n, nb, scale=None):
    ys = []
    for _ in range(nb):
        y = rng.normal(size=n)
        if scale is not None:
            y = y * scale
        ys.append(y.astype(np.float32).astype(np.float64))
    return ys


def context_of(Ctx, g, brs, stats=None):
    m = g.shape[0]
    specs = [dict(snps=np.arange(m, dtype=np.int32), branch=br, y=np.zeros(g.shape[1])) for br in brs]
    ctx = build_context(Ctx, g, specs, stats=stats)
    return ctx


def oracle_x(ctx, g):
    mu, sd = ctx.genotype_stats()
    return x_std(g, mu, sd)


def check_all(ctx, ref, ys, label):
    """every branch's gradient, rss and prediction of one packed launch against the oracle; returns them"""
    nb = len(ref)
    for b in range(nb):
        ctx.set_target(b, ys[b])
    grads, rss = ctx.log_density_gradient_many(list(range(nb)))
    preds = ctx.predict_many(list(range(nb)))
    eg = [norm_rel(grads[b], ref[b]["grad"]) for b in range(nb)]
    # a prediction that is exactly 0 (part 3) has no norm to be relative to: absolute there
    ep = [norm_rel(preds[b], ref[b]["f"]) if np.any(ref[b]["f"]) else float(np.max(np.abs(preds[b]))) for b in range(nb)]
    er = [abs(rss[b] - ref[b]["rss"]) / max(1.0, abs(ref[b]["rss"])) for b in range(nb)]
    print(f"{label}: worst of {nb} branches: gradient {max(eg):.2e} (branch {int(np.argmax(eg))}), "
          f"prediction {max(ep):.2e}, rss {max(er):.2e}")
    for b in range(nb):
        assert eg[b] < TOL, (label, b, eg[b])
        assert scalar_close(rss[b], ref[b]["rss"]), (label, b, rss[b], ref[b]["rss"])
        assert ep[b] < TOL, (label, b, ep[b])
    return grads, rss


@pytest.mark.parametrize("name", list(SHAPES))
def test_long_items_match_oracle(Ctx, monkeypatch, name):
    """part 1: standard-normal targets; the packed launch is bitwise repeatable, and a branch evaluated alone
    (another plan: its own items only) agrees with its packed result to f32 rounding (1e-6: a few ulps of the
    fixed-order partial sums)"""
    long_item_env(monkeypatch, SHAPES[name][3])
    g, brs = shape_case(name)
    ctx = context_of(Ctx, g, brs)
    assert all(ctx.kernel_path(b) == "fused_large" for b in range(NB))
    ys = f32_targets(np.random.default_rng(101), N, NB)
    ref = reference(brs, oracle_x(ctx, g), ys)
    grads, rss = check_all(ctx, ref, ys, f"part 1 {name}")
    again, rss_again = ctx.log_density_gradient_many(list(range(NB)))
    assert all(np.array_equal(a, b) for a, b in zip(grads, again)) and np.array_equal(rss, rss_again)
    for b in (0, 31, 63):
        g1, r1 = ctx.log_density_gradient(b)
        e1 = norm_rel(g1, grads[b])
        print(f"part 1 {name}: branch {b} alone against packed {e1:.2e}")
        assert e1 < 1e-6 and scalar_close(r1, rss[b], 1e-6), (b, e1, r1, rss[b])
        assert norm_rel(g1, ref[b]["grad"]) < TOL and scalar_close(r1, ref[b]["rss"]), b
    ctx.close()


@pytest.mark.parametrize("name", list(SHAPES))
def test_scale_grows_twice_inside_every_item(Ctx, monkeypatch, name):
    """part 2: targets 2^0, 2^10, 2^20 times standard normal by tile: every item grows its delta0 scale by 2^10
    twice and has to rescale the digit sums of its earlier tiles each time"""
    long_item_env(monkeypatch, SHAPES[name][3])
    g, brs = shape_case(name)
    ctx = context_of(Ctx, g, brs)
    ys = f32_targets(np.random.default_rng(202), N, NB, tile_scale(N))
    ref = reference(brs, oracle_x(ctx, g), ys)
    check_all(ctx, ref, ys, f"part 2 {name}")
    ctx.close()


@pytest.mark.parametrize("name", list(SHAPES))
def test_column_scale_unset_then_set_while_others_grow(Ctx, monkeypatch, name):
    """part 2's designed case: column 2's delta0 is exactly 0 in the tiles with (i // 64) % 3 == 0, so an item
    that starts on one sets the scales of columns 0, 1 and 3 first and column 2's a tile later, while the
    others grow; in an item's later tiles of that kind column 2 contributes zero digits at a set scale"""
    long_item_env(monkeypatch, SHAPES[name][3])
    g, brs = designed_case(name)
    m = g.shape[0]
    ctx = context_of(Ctx, g, brs, stats=(np.zeros(m), np.ones(m)))
    X = g.T.astype(np.float64)
    dead = (np.arange(N) // 64) % 3 == 0
    z2 = X @ brs[0].weights[0][:, 2] + brs[0].biases[0][2]
    assert np.all(z2[dead] < -10.0) and np.any(z2[~dead] > 0.0)  # the design holds
    ys = f32_targets(np.random.default_rng(303), N, NB, tile_scale(N))
    ref = reference(brs, X, ys)
    check_all(ctx, ref, ys, f"designed {name}")
    ctx.close()


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("name", ["fx"] + list(SHAPES))
def test_coherent_backward_digit_sums(Ctx, monkeypatch, name, pattern):
    """part 3: every delta0 digit at its largest and of one sign, so the int32 dW0 digit sums grow linearly
    over an item's tiles: the carry out of the top digit, field 3's correction and the exact combine"""
    if name == "fx":
        monkeypatch.setenv("BANN_TARGET_ITEMS", "1")
        monkeypatch.setenv("BANN_SOLO", "0")
        m, n, nb, path = 512, 16384, 3, "fused"
    else:
        long_item_env(monkeypatch, SHAPES[name][3])
        m, n, nb, path = SHAPES[name][0], N, NB, "fused_large"
    g, brs = coherent_case(m, n, nb, pattern)
    ctx = context_of(Ctx, g, brs, stats=(np.zeros(m), np.ones(m)))
    assert all(ctx.kernel_path(b) == path for b in range(nb))
    X = g.T.astype(np.float64)
    for sign in (1.0, -1.0):
        ys = coherent_targets(n, nb, sign)
        assert all(np.array_equal(y, y.astype(np.float32)) for y in ys)  # f32 holds them exactly
        ref = reference(brs, X, ys)
        check_all(ctx, ref, ys, f"part 3 {name} {pattern} y {'+' if sign > 0 else '-'}")
    ctx.close()


# ---------------------------------------------------------------------------------------------- code 3
CODE3_PATHS = {"fx": (100, [4, 4, 1], "fused"), "fxl": (577, [4, 1], "fused_large"),
               "fxh": (1100, [4, 4, 1], "fused_large"), "wx": (128, [32, 32, 1], "wide"),
               "gx": (100, [50, 50, 1], "layered")}
CODE3_N = 300


def code3_cohort(where):
    """a called cohort with a fifth of its calls replaced by the 2-bit value 3: at individuals 3 mod 4 only
    ("field3") or at any individual ("anywhere")"""
    rng = np.random.default_rng(404)
    M = max(m for m, _, _ in CODE3_PATHS.values())
    g = O.synthetic_genotypes(rng, CODE3_N, M)
    hit = rng.random(size=g.shape) < 0.2
    if where == "field3":
        hit &= (np.arange(CODE3_N) % 4 == 3)[None, :]
    g[hit] = 3
    return g


def code3_spec(rng, kind):
    m, widths, _ = CODE3_PATHS[kind]
    br = f32_branch(O.random_branch(rng, m, widths, prior="ridge_ard", act="tanh"))
    return dict(snps=np.arange(m, dtype=np.int32), branch=br,
                y=rng.normal(size=CODE3_N).astype(np.float32).astype(np.float64))


@pytest.mark.parametrize("where", ["field3", "anywhere"])
def test_code_three_counts_as_three_or_is_refused(Ctx, where):
    """part 4: wx and gx read an uploaded 3 as 3.0 (prediction, gradient, forward_feed against the oracle at
    the device's own mu and sigma); the fx family's tile images cannot hold it in field 3, and bann_finalize
    refuses the cohort for every fx, fxl or fxh branch, alone or beside others -- wherever its 3s sit: the
    flag is the cohort's"""
    from bann import BannError
    g = code3_cohort(where)
    rng = np.random.default_rng(405)
    specs = {kind: code3_spec(rng, kind) for kind in CODE3_PATHS}
    ctx = build_context(Ctx, g, [specs["wx"], specs["gx"]])
    mu, sd = ctx.genotype_stats()
    for b, kind in enumerate(("wx", "gx")):
        s = specs[kind]
        assert ctx.kernel_path(b) == CODE3_PATHS[kind][2]
        assert np.array_equal(ctx.download_genotypes(s["snps"]), g[s["snps"]])
        X = x_std(g[s["snps"]], mu[s["snps"]], sd[s["snps"]])
        gw, gb, rss_ref = O.log_density_gradient(s["branch"], X, s["y"])
        grad, rss = ctx.log_density_gradient(b)
        eg, ep = norm_rel(grad, O.param_vec(gw, gb)), norm_rel(ctx.predict(b), O.predict(s["branch"], X))
        print(f"code 3 {where} {kind}: gradient {eg:.2e}, prediction {ep:.2e}")
        assert eg < TOL and ep < TOL and scalar_close(rss, rss_ref), (kind, eg, ep, rss, rss_ref)
        pre, act = ctx.forward_feed(b)
        opre, oact = O.forward_feed(s["branch"], X)
        for a, oa in zip(pre + act, opre + oact):
            assert a.shape == oa.shape and norm_rel(a, oa) < TOL, kind
    ctx.close()
    for kinds in (["fx"], ["fxl"], ["fxh"], ["wx", "fx", "gx"]):
        with pytest.raises(BannError) as err:
            build_context(Ctx, g, [specs[k] for k in kinds]).close()
        assert err.value.code == -5 and "3" in str(err.value), (kinds, str(err.value))
    # with the fused kernels off every branch is gx, which holds the value: no refusal
    ctx = build_context(Ctx, g, [specs["fx"], specs["fxl"]], fused=False)
    assert all(ctx.kernel_path(b) == "layered" for b in range(2))
    s = specs["fx"]
    X = x_std(g[s["snps"]], mu[s["snps"]], sd[s["snps"]])
    assert norm_rel(ctx.predict(0), O.predict(s["branch"], X)) < TOL
    ctx.close()
    # the same cohort without its 3s is not refused
    clean = np.where(g == 3, 0, g).astype(np.int8)
    ctx = build_context(Ctx, clean, [specs["fx"]])
    assert ctx.kernel_path(0) == "fused"
    ctx.close()
