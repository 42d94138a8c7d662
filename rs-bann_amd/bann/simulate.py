"""Starting a model and simulating phenotypes, without the reference installed.

  new_net      rs-bann train-new's construction up to "Training net" (rs-bann.rs:1093-1107): the
               branches of a grouping added by the width rules, the net built on the device
  simulate_y   rs-bann simulate-y (rs-bann.rs:374-517): such a net, the train and test cohorts
               predicted, Gaussian noise sized by a heritability, the reference's output files
"""
from __future__ import annotations

import json
import os
from typing import Optional, Sequence, Tuple

import numpy as np

from ._lib import BannError, load_library
from .arch import InitConfig, layer_widths
from .context import BannContext
from .io import format_f32, read_grouping, write_phen
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
    """simulate-y's directory name without the replicate suffix (rs-bann.rs:388-404)."""
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


def simulate_y(bfile_train: str, bfile_test: str, groups, prior: str, activation: str, depth: int, outdir: str,
               heritability: float = 1.0, num_effective: Optional[int] = None,
               proportion_effective: Optional[float] = None, init_param_variance: Optional[float] = None,
               init_gamma: Optional[Sequence[float]] = None, seed: int = 0, device: int = 0) -> str:
    """rs-bann simulate-y.  Writes outdir/<name>_rep<ix>/ with model.bin, model.params, train.phen,
    test.phen, train_phen_stats.json, test_phen_stats.json and args.json, and returns that directory.
    The draws come from ``seed`` (the reference seeds from entropy); the train noise is drawn from
    seed and the test noise from seed + 1."""
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
        args = {"bfile_train": bfile_train, "bfile_test": bfile_test,
                "groups": os.fspath(groups) if isinstance(groups, (str, os.PathLike)) else None,
                "model_type": PRIOR_NAMES[prior], "activation_function": ACTIVATION_NAMES[activation],
                "depth": int(depth), "outdir": outdir, "proportion_effective": proportion_effective,
                "num_effective": num_effective, "init_param_variance": init_param_variance,
                "init_gamma_shape": None if gamma is None else gamma[0],
                "init_gamma_scale": None if gamma is None else gamma[1], "heritability": heritability,
                "json_data": False, "debug": False, "seed": int(seed)}
        with open(os.path.join(path, "args.json"), "w") as f:
            json.dump(args, f, indent=2)
        net.close()
    finally:
        train.close()
        test.close()
    return path
