"""Starting a model and simulating phenotypes, without the reference installed.

  new_net      rs-bann train-new's construction up to "Training net" (rs-bann.rs:1093-1107): the
               branches of a grouping added by the width rules, the net built on the device
  simulate_y   rs-bann simulate-y (rs-bann.rs:374-517): such a net, the train and test cohorts
               predicted, Gaussian noise sized by a heritability, the reference's output files
  simulate_y_linear   simulate-y --model-type Linear (rs-bann.rs:519-644): drawn linear effects scored
               on both cohorts from the resident images, several replicates from one genotype pass
  simulate_xy  rs-bann simulate-xy, network (rs-bann.rs:793-960) or linear (646-774): the two cohorts
               generated on the device and written back as .bed / .dims / .groups
"""
from __future__ import annotations

import json
import os
from typing import Optional, Sequence, Tuple

import numpy as np

from ._lib import BannError, load_library
from .arch import InitConfig, layer_widths
from .context import BannContext
from .io import format_f32, read_grouping, uniform_grouping, write_grouping, write_phen
from .net import VAGUE, Net

# ModelType / ActivationFunction as the reference prints them (Display = Debug of the variant)
PRIOR_NAMES = {"ridge_ard": "RidgeARD", "ridge_base": "RidgeBase", "lasso_ard": "LassoARD",
               "lasso_base": "LassoBase", "std_normal": "StdNormal"}
ACTIVATION_NAMES = {"tanh": "Tanh", "relu": "ReLU", "leaky_relu": "LeakyReLU", "silu": "SiLU",
                    "identity": "Identity"}


def _groups(groups):
    return read_grouping(groups) if isinstance(groups, (str, os.PathLike)) else [np.asarray(g, np.int32) for g in groups]


def _context(bfile: str, groups, prior: str, activation: str, depth: int, hidden, summary, device: int) -> BannContext:
    ctx = BannContext(device)
    ctx.load_bed(bfile)
    for g in groups:
        ctx.add_branch(g, layer_widths(len(g), depth, hidden, summary), activation, prior)
    ctx.finalize()
    return ctx


def new_net(ctx_or_bfile, groups, prior: str = "ridge_ard", activation: str = "tanh", depth: int = 1,
            hidden: Tuple = ("fraction", 0.5), summary: Tuple = ("fraction", 1.0),
            hyperparams: Tuple = (VAGUE, VAGUE, VAGUE), fixed_param_precision: Optional[float] = None,
            seed: int = 0, device: int = 0) -> Net:
    """The net rs-bann train-new builds before it trains (train-new's defaults: hidden width half the
    markers, summary width like the hidden one, vague hyperparameters).  ctx_or_bfile: a PLINK stem,
    or a BannContext with its cohort loaded and no branches yet.  groups: a grouping file or marker
    index lists.  The caller goes on with ``train`` / ``train_network``; the context is ``net._ctx``."""
    gl = _groups(groups)
    if isinstance(ctx_or_bfile, BannContext):
        ctx = ctx_or_bfile
        for g in gl:
            ctx.add_branch(g, layer_widths(len(g), depth, hidden, summary), activation, prior)
        ctx.finalize()
    else:
        ctx = _context(os.fspath(ctx_or_bfile), gl, prior, activation, depth, hidden, summary, device)
    net = Net(ctx, hyperparams, seed)
    net.init(InitConfig(fixed_precision=fixed_param_precision), seed)
    return net


def _rust_debug_f32(v: float) -> str:
    """{:?} of an f32 in the range the directory names meet: the shortest digits, always a fraction part"""
    t = format_f32(v)
    return t if "." in t or not t.lstrip("-").isdigit() else t + ".0"


def output_dir_name(prior: str, activation: str, depth: int, heritability: float,
                    num_effective: Optional[int] = None, proportion_effective: Optional[float] = None,
                    init_param_variance: Optional[float] = None,
                    init_gamma: Optional[Tuple[float, float]] = None) -> str:
    """simulate-y's directory name without the replicate suffix (rs-bann.rs:388-404); prior "linear":
    the linear simulator's, model type and heritability alone in front (rs-bann.rs:530-543)."""
    if prior == "linear":
        name = f"Linear_h{format_f32(heritability)}"
    else:
        name = f"{PRIOR_NAMES[prior]}_{ACTIVATION_NAMES[activation]}_d{int(depth)}_h{format_f32(heritability)}"
    if num_effective is not None:
        name += f"_me{int(num_effective)}"
    elif proportion_effective is not None:
        name += f"_pe{_rust_debug_f32(proportion_effective)}"
    if init_param_variance is not None:
        name += f"_v{_rust_debug_f32(init_param_variance)}"
    elif init_gamma is not None:
        name += f"_k{_rust_debug_f32(init_gamma[0])}_s{_rust_debug_f32(init_gamma[1])}"
    return name


def replicate_dir(parent: str, name: str) -> str:
    """set_replicate_ix (rs-bann.rs:776-787): parent/name_rep<ix>, the first ix >= 1 that does not exist."""
    ix = 1
    while os.path.exists(os.path.join(parent, f"{name}_rep{ix}")):
        ix += 1
    return os.path.join(parent, f"{name}_rep{ix}")


def write_phen_stats(path: str, stats: dict) -> None:
    lib = load_library()
    rc = lib.bann_phen_stats_write(os.fspath(path).encode(), stats["mean"], stats["variance"], stats["env_variance"])
    if rc != 0:
        raise BannError(rc, lib.bann_io_last_error().decode())


def _json_f32(v) -> str:
    """an f32 as a JSON number: format_f32's digits, always with a fraction part.  serde_json switches
    to exponents where this keeps positional digits; the parsed values are identical."""
    t = format_f32(v)
    if t in ("NaN", "inf", "-inf"):
        return "null"
    return t if "." in t else t + ".0"


def write_phen_json(path: str, y) -> None:
    """Phenotypes::to_json (data/phenotypes.rs:38-40): {"y":[...]} on one line"""
    with open(path, "w") as f:
        f.write('{"y":[' + ",".join(_json_f32(v) for v in np.asarray(y, np.float32)) + "]}")


def write_json_data(path: str, g_train, g_test, y_train, y_test) -> None:
    """the four files of --json-data (rs-bann.rs:636-641)"""
    write_phen_json(os.path.join(path, "genetic_values_test.json"), g_test)
    write_phen_json(os.path.join(path, "genetic_values_train.json"), g_train)
    write_phen_json(os.path.join(path, "phen_train.json"), y_train)
    write_phen_json(os.path.join(path, "phen_test.json"), y_test)


def linear_model_line(num_markers_per_branch: Sequence[int], effects) -> str:
    """the LinearModel (linear_model.rs:102-107) as one serde_json line plus the newline: model.params
    of the linear simulators.  effects: the E = sum of the branch sizes values, branch by branch."""
    sizes = [int(s) for s in num_markers_per_branch]
    eff = np.asarray(effects, np.float32).ravel()
    if eff.size != sum(sizes):
        raise ValueError("one effect per entry")
    rows, o = [], 0
    for s in sizes:
        rows.append("[" + ",".join(_json_f32(v) for v in eff[o:o + s]) + "]")
        o += s
    return ('{"num_branches":%d,"num_markers_per_branch":[%s],"effects":[%s]}\n'
            % (len(sizes), ",".join(str(s) for s in sizes), ",".join(rows)))


def xy_output_dir_name(prior: str, activation: Optional[str], num_branches: int, hidden_layer_width: int,
                       summary_layer_width: Optional[int], depth: int, num_markers_per_branch: int,
                       num_individuals: int, heritability: float, num_effective: Optional[int] = None,
                       proportion_effective: Optional[float] = None, init_param_variance: Optional[float] = None,
                       init_gamma: Optional[Tuple[float, float]] = None) -> str:
    """simulate-xy's directory name without the replicate suffix (rs-bann.rs:803-827); prior "linear":
    the linear variant's (rs-bann.rs:653-676), which has no activation and appends the initialisation
    as "v_1.0" / "k_2.0s_0.5" with no underscore in front -- the reference's quirk, kept."""
    linear = prior == "linear"
    head = "Linear" if linear else f"{PRIOR_NAMES[prior]}_{ACTIVATION_NAMES[activation]}"
    ws = hidden_layer_width if summary_layer_width is None else summary_layer_width
    name = (f"{head}_b{int(num_branches)}_wh{int(hidden_layer_width)}_ws{int(ws)}_d{int(depth)}"
            f"_m{int(num_markers_per_branch)}_n{int(num_individuals)}_h{format_f32(heritability)}")
    if num_effective is not None:
        name += f"_me{int(num_effective)}"
    elif proportion_effective is not None:
        name += f"_pe{_rust_debug_f32(proportion_effective)}"
    v, k, s = ("v_", "k_", "s_") if linear else ("_v", "_k", "_s")
    if init_param_variance is not None:
        name += f"{v}{_rust_debug_f32(init_param_variance)}"
    elif init_gamma is not None:
        name += f"{k}{_rust_debug_f32(init_gamma[0])}{s}{_rust_debug_f32(init_gamma[1])}"
    return name


def _write_phenotypes(path: str, y_train, st_train, y_test, st_test) -> None:
    write_phen_stats(os.path.join(path, "test_phen_stats.json"), st_test)
    write_phen_stats(os.path.join(path, "train_phen_stats.json"), st_train)
    write_phen(os.path.join(path, "train.phen"), y_train)
    write_phen(os.path.join(path, "test.phen"), y_test)


def _write_args(path: str, args: dict) -> None:
    with open(os.path.join(path, "args.json"), "w") as f:
        json.dump(args, f, indent=2)


def simulate_y_linear(bfile_train: str, bfile_test: str, groups, outdir: str, heritability: float = 1.0,
                      num_effective: Optional[int] = None, proportion_effective: Optional[float] = None,
                      seed: int = 0, json_data: bool = False, device: int = 0, replicates: int = 1):
    """rs-bann simulate-y --model-type Linear (rs-bann.rs:519-644).  Writes outdir/Linear_h..._rep<ix>/
    with model.params (the LinearModel line), train.phen, test.phen, the two *_phen_stats.json and
    args.json (json_data: the four JSON files too), and returns that directory.  The effects come from
    ``seed``, the train noise from seed and the test noise from seed + 1.  num_effective counts over the
    entries of the whole model (linear_model.rs:53-58).
    replicates = R > 1: R directories from one score pass per cohort, replicate r with seed + 2 r, its
    files byte-identical to a single call with that seed; the list of directories is returned."""
    if not 0.0 <= heritability <= 1.0:
        raise ValueError("Heritability must be within [0, 1].")
    R = int(replicates)
    if R < 1:
        raise ValueError("replicates must be at least 1")
    name = output_dir_name("linear", None, 0, heritability, num_effective, proportion_effective)
    gl = _groups(groups)
    sizes = [len(g) for g in gl]
    E = sum(sizes)
    train, test = BannContext(device), BannContext(device)
    paths = []
    try:
        train.load_bed(bfile_train)
        test.load_bed(bfile_test)
        seeds = [int(seed) + 2 * r for r in range(R)]
        eff = np.stack([train.linear_effects(E, heritability, num_effective, proportion_effective, s)[0] for s in seeds])
        y_tr, g_tr, st_tr = train.linear_simulate_y(gl, eff, heritability, seeds, return_g=True)
        y_te, g_te, st_te = test.linear_simulate_y(gl, eff, heritability, [s + 1 for s in seeds], return_g=True)
        for r in range(R):
            path = replicate_dir(outdir, name)
            os.makedirs(path)
            with open(os.path.join(path, "model.params"), "w") as f:
                f.write(linear_model_line(sizes, eff[r]))
            _write_phenotypes(path, y_tr[r], st_tr[r], y_te[r], st_te[r])
            if json_data:
                write_json_data(path, g_tr[r], g_te[r], y_tr[r], y_te[r])
            _write_args(path, {"bfile_train": bfile_train, "bfile_test": bfile_test,
                               "groups": os.fspath(groups) if isinstance(groups, (str, os.PathLike)) else None,
                               "model_type": "Linear", "activation_function": None, "depth": 0, "outdir": outdir,
                               "proportion_effective": proportion_effective, "num_effective": num_effective,
                               "init_param_variance": None, "init_gamma_shape": None, "init_gamma_scale": None,
                               "heritability": heritability, "json_data": bool(json_data), "debug": False,
                               "seed": seeds[r]})
            paths.append(path)
    finally:
        train.close()
        test.close()
    return paths[0] if R == 1 else paths


def simulate_xy(prior: str, activation: Optional[str], num_branches: int, num_markers_per_branch: int,
                num_individuals: int, hidden_layer_width: int, summary_layer_width: Optional[int], depth: int,
                outdir: str, heritability: float = 1.0, num_effective: Optional[int] = None,
                proportion_effective: Optional[float] = None, init_param_variance: Optional[float] = None,
                init_gamma: Optional[Sequence[float]] = None, seed: int = 0, json_data: bool = False,
                device: int = 0, max_attempts: int = 16) -> str:
    """rs-bann simulate-xy (rs-bann.rs:793-960), and with prior "linear" its linear variant (646-774):
    a train and a test cohort generated on the device from shared allele frequencies, phenotypes
    under a freshly drawn network or linear model.  Writes outdir/<name>_rep<ix>/ with train.bed /
    .dims / .groups, test.*, model.params (and model.bin for a network), the phenotype and stats files
    and args.json, and returns that directory.
    The allele frequencies are 0.5 u from numpy.random.default_rng(seed) on the host, the cohorts have
    seeds seed and seed + 1, the model seed, the noise seed and seed + 1.  The network variant redoes
    everything with seed + 2 attempt while a residual variance is below 0.01 and heritability != 1
    (rs-bann.rs:912-918), max_attempts times at most."""
    if not 0.0 <= heritability <= 1.0:
        raise ValueError("Heritability must be within [0, 1].")
    linear = prior == "linear"
    gamma = None if init_gamma is None else (float(init_gamma[0]), float(init_gamma[1]))
    nb, mpb, n = int(num_branches), int(num_markers_per_branch), int(num_individuals)
    M = nb * mpb
    path = replicate_dir(outdir, xy_output_dir_name(prior, activation, nb, hidden_layer_width, summary_layer_width,
                                                    depth, mpb, n, heritability, num_effective, proportion_effective,
                                                    init_param_variance, gamma))
    gl = uniform_grouping(nb, mpb)
    args = {"outdir": outdir, "model_type": "Linear" if linear else PRIOR_NAMES[prior],
            "activation_function": None if activation is None else ACTIVATION_NAMES[activation],
            "num_markers_per_branch": mpb, "num_branches": nb, "num_individuals": n,
            "hidden_layer_width": int(hidden_layer_width), "branch_depth": int(depth),
            "proportion_effective": proportion_effective, "num_effective": num_effective,
            "summary_layer_width": summary_layer_width, "init_param_variance": init_param_variance,
            "init_gamma_shape": None if gamma is None else gamma[0],
            "init_gamma_scale": None if gamma is None else gamma[1], "heritability": heritability,
            "json_data": bool(json_data), "seed": int(seed)}

    def cohorts(s):
        mafs = (0.5 * np.random.default_rng(s).random(M)).astype(np.float32)
        tr, te = BannContext(device), BannContext(device)
        tr.synthetic_genotypes(n, M, s, mafs)
        te.synthetic_genotypes(n, M, s + 1, mafs)
        return tr, te

    def finish(tr, te, y_tr, g_tr, st_tr, y_te, g_te, st_te):
        for c, stem in ((tr, "train"), (te, "test")):
            c.save_bed(os.path.join(path, stem))
            write_grouping(os.path.join(path, stem + ".groups"), gl)
        _write_phenotypes(path, y_tr, st_tr, y_te, st_te)
        if json_data:
            write_json_data(path, g_tr, g_te, y_tr, y_te)
        _write_args(path, args)

    if linear:
        train, test = cohorts(int(seed))
        try:
            eff, _ = train.linear_effects(M, heritability, num_effective, proportion_effective, seed)
            y_tr, g_tr, st_tr = train.linear_simulate_y(gl, eff, heritability, seed, return_g=True)
            y_te, g_te, st_te = test.linear_simulate_y(gl, eff, heritability, seed + 1, return_g=True)
            os.makedirs(path)
            with open(os.path.join(path, "model.params"), "w") as f:
                f.write(linear_model_line([mpb] * nb, eff))
            finish(train, test, y_tr, g_tr, st_tr, y_te, g_te, st_te)
        finally:
            train.close()
            test.close()
        return path

    widths = layer_widths(mpb, depth, ("fixed", int(hidden_layer_width)),
                          ("like_hidden",) if summary_layer_width is None else ("fixed", int(summary_layer_width)))
    hp = (VAGUE, VAGUE, VAGUE) if gamma is None else (gamma, gamma, (1.0, 1.0))
    cfg = InitConfig(variance=None if gamma is not None else init_param_variance, gamma=gamma,
                     num_effective=num_effective, proportion_effective=proportion_effective)
    for attempt in range(int(max_attempts)):
        s = int(seed) + 2 * attempt
        train, test = cohorts(s)
        net = None
        try:
            for c in (train, test):
                for g in gl:
                    c.add_branch(g, widths, activation, prior)
                c.finalize()
            net = Net(train, hp, s)
            net.init(cfg, s)
            y_tr, st_tr = net.simulate_y(heritability, s, None)
            y_te, st_te = net.simulate_y(heritability, s + 1, test)
            if heritability != 1.0 and (st_tr["env_variance"] < 0.01 or st_te["env_variance"] < 0.01):
                continue
            os.makedirs(path)
            net.save(os.path.join(path, "model.bin"))
            net.write_params(os.path.join(path, "model.params"))
            g_tr, g_te = (net.predict(), net.predict(test)) if json_data else (None, None)
            finish(train, test, y_tr, g_tr, st_tr, y_te, g_te, st_te)
            return path
        finally:
            if net is not None:
                net.close()
            train.close()
            test.close()
    raise RuntimeError(f"simulate_xy: a residual variance stayed below 0.01 in {int(max_attempts)} attempts "
                       "(rs-bann.rs:912-918 would go on drawing)")


def simulate_y(bfile_train: str, bfile_test: str, groups, prior: str, activation: str, depth: int, outdir: str,
               heritability: float = 1.0, num_effective: Optional[int] = None,
               proportion_effective: Optional[float] = None, init_param_variance: Optional[float] = None,
               init_gamma: Optional[Sequence[float]] = None, seed: int = 0, device: int = 0,
               json_data: bool = False) -> str:
    """rs-bann simulate-y.  Writes outdir/<name>_rep<ix>/ with model.bin, model.params, train.phen,
    test.phen, train_phen_stats.json, test_phen_stats.json and args.json, and returns that directory.
    The draws come from ``seed`` (the reference seeds from entropy); the train noise is drawn from
    seed and the test noise from seed + 1.  json_data: also the four JSON files of rs-bann.rs:636-641."""
    if not 0.0 <= heritability <= 1.0:
        raise ValueError("Heritability must be within [0, 1].")
    gamma = None if init_gamma is None else (float(init_gamma[0]), float(init_gamma[1]))
    path = replicate_dir(outdir, output_dir_name(prior, activation, depth, heritability, num_effective,
                                                 proportion_effective, init_param_variance, gamma))
    gl = _groups(groups)
    rules = (("fraction", 0.5), ("like_hidden",))
    train = _context(bfile_train, gl, prior, activation, depth, *rules, device)
    test = _context(bfile_test, gl, prior, activation, depth, *rules, device)
    try:
        # gamma init: the dense and summary hyperparameters are the init pair, the output pair (1, 1)
        hp = (VAGUE, VAGUE, VAGUE) if gamma is None or init_param_variance is not None else (gamma, gamma, (1.0, 1.0))
        net = Net(train, hp, seed)
        net.init(InitConfig(variance=init_param_variance, gamma=None if init_param_variance is not None else gamma,
                            num_effective=num_effective, proportion_effective=proportion_effective), seed)
        os.makedirs(path)
        net.save(os.path.join(path, "model.bin"))
        net.write_params(os.path.join(path, "model.params"))
        y_train, st_train = net.simulate_y(heritability, seed, None)
        y_test, st_test = net.simulate_y(heritability, seed + 1, test)
        write_phen_stats(os.path.join(path, "test_phen_stats.json"), st_test)
        write_phen_stats(os.path.join(path, "train_phen_stats.json"), st_train)
        write_phen(os.path.join(path, "train.phen"), y_train)
        write_phen(os.path.join(path, "test.phen"), y_test)
        if json_data:
            write_json_data(path, net.predict(), net.predict(test), y_train, y_test)
        args = {"bfile_train": bfile_train, "bfile_test": bfile_test,
                "groups": os.fspath(groups) if isinstance(groups, (str, os.PathLike)) else None,
                "model_type": PRIOR_NAMES[prior], "activation_function": ACTIVATION_NAMES[activation],
                "depth": int(depth), "outdir": outdir, "proportion_effective": proportion_effective,
                "num_effective": num_effective, "init_param_variance": init_param_variance,
                "init_gamma_shape": None if gamma is None else gamma[0],
                "init_gamma_scale": None if gamma is None else gamma[1], "heritability": heritability,
                "json_data": bool(json_data), "debug": False, "seed": int(seed)}
        with open(os.path.join(path, "args.json"), "w") as f:
            json.dump(args, f, indent=2)
        net.close()
    finally:
        train.close()
        test.close()
    return path
