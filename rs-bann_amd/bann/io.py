"""Files on either side of the hot path, through the library's host-only C ABI
(no device needed): PLINK dims, marker groupings, bincode phenotypes.

  bed_dims            BedDims (io/dims.rs:15-34)
  read_grouping       ExternalGrouping::from_file (group/external.rs:15-60)
  uniform_grouping    UniformGrouping::new (group/uniform.rs:11-23)
  read_phen/write_phen Phenotypes::from_file / to_file (data/phenotypes.rs:28-36)
  read_bim            .bim chromosome index and position per marker
  read_plink_ld_graph CorrGraph::from_plink_ld (group/centered.rs:54-89)
  centered_grouping   CorrGraph::centered_grouping (group/centered.rs:91-133)
  write_grouping      MarkerGrouping::to_file (group/grouping.rs:16-31)
  group_by_ld         rs-bann group-by-ld with the LD taken from the context's cohort on the device
  encode_bed_payload  int8 genotypes with -1 for a missing call -> the variant-major .bed payload
  read_fam            the lines of a .fam, verbatim, and their count
  split_indices / kfold_indices   ascending index lists of a train / test split and of K folds
  split_train_test    scripts/split_train_test.sh without PLINK: one load, two device subsets, two filesets
  fill_missing_a2     scripts/fill_missing_a2.sh without PLINK
  list_model_files / write_predictions_csv   the model listing and the CSV records of
                      rs-bann predict (rs-bann.rs:288-311); pure Python
  write_branch_r2_csv / write_population_effect_sizes_json   the outputs of rs-bann branch-r2
                      (rs-bann.rs:128-166) and population-effect-sizes (314-372); pure Python
"""
from __future__ import annotations

import ctypes as C
import json
import os
import shutil
from typing import List

import numpy as np

from ._lib import BannError, load_library


def _chk(rc, what):
    if rc != 0:
        detail = load_library().bann_io_last_error().decode()
        raise BannError(rc, f"{what}: {detail}" if detail else what)


def bed_dims(stem: str):
    """(n, num_markers) of a PLINK fileset stem: stem.dims, else the .fam / .bim line counts."""
    n, m = C.c_int64(), C.c_int64()
    _chk(load_library().bann_bed_dims(stem.encode(), C.byref(n), C.byref(m)), f"bann_bed_dims({stem})")
    return n.value, m.value


def read_grouping(path: str) -> List[np.ndarray]:
    """marker index lists of an external grouping file (one int32 array per group)."""
    lib = load_library()
    G, E = C.c_int32(), C.c_int64()
    _chk(lib.bann_grouping_read(path.encode(), C.byref(G), C.byref(E), None, None), f"bann_grouping_read({path})")
    off = np.zeros(G.value + 1, np.int64)
    mk = np.zeros(max(E.value, 1), np.int32)
    _chk(lib.bann_grouping_read(path.encode(), C.byref(G), C.byref(E), off.ctypes.data_as(C.POINTER(C.c_int64)),
                                mk.ctypes.data_as(C.POINTER(C.c_int32))), f"bann_grouping_read({path})")
    return [mk[off[g]:off[g + 1]].copy() for g in range(G.value)]


def uniform_grouping(num_groups: int, group_size: int) -> List[np.ndarray]:
    off = np.zeros(num_groups + 1, np.int64)
    mk = np.zeros(num_groups * group_size, np.int32)
    _chk(load_library().bann_grouping_uniform(num_groups, group_size, off.ctypes.data_as(C.POINTER(C.c_int64)),
                                              mk.ctypes.data_as(C.POINTER(C.c_int32))), "bann_grouping_uniform")
    return [mk[off[g]:off[g + 1]].copy() for g in range(num_groups)]


def read_bim(path: str):
    """(chrom, bp) of a .bim: int32 chromosome index by first appearance, int64 position."""
    lib = load_library()
    m = C.c_int64()
    _chk(lib.bann_bim_read(path.encode(), C.byref(m), None, None), f"bann_bim_read({path})")
    chrom = np.zeros(m.value, np.int32)
    bp = np.zeros(m.value, np.int64)
    _chk(lib.bann_bim_read(path.encode(), C.byref(m), chrom.ctypes.data_as(C.POINTER(C.c_int32)),
                           bp.ctypes.data_as(C.POINTER(C.c_int64))), f"bann_bim_read({path})")
    return chrom, bp


def read_plink_ld_graph(ld_path: str, bim_path: str):
    """(offsets, neighbours): the symmetric CSR graph of a PLINK --r2 table over the .bim's markers."""
    lib = load_library()
    m, e = C.c_int64(), C.c_int64()
    what = f"bann_ld_graph_read_plink({ld_path}, {bim_path})"
    _chk(lib.bann_ld_graph_read_plink(ld_path.encode(), bim_path.encode(), C.byref(m), C.byref(e), None, None), what)
    off = np.zeros(m.value + 1, np.int64)
    nb = np.zeros(max(2 * e.value, 1), np.int32)
    _chk(lib.bann_ld_graph_read_plink(ld_path.encode(), bim_path.encode(), C.byref(m), C.byref(e),
                                      off.ctypes.data_as(C.POINTER(C.c_int64)),
                                      nb.ctypes.data_as(C.POINTER(C.c_int32))), what)
    return off, nb[:2 * e.value]


def _csr(groups):
    off = np.zeros(len(groups) + 1, np.int64)
    off[1:] = np.cumsum([len(g) for g in groups])
    mk = np.zeros(max(int(off[-1]), 1), np.int32)
    for g, members in enumerate(groups):
        mk[off[g]:off[g + 1]] = members
    return off, mk


def centered_grouping(offsets, neighbours, min_group_size: int = 1):
    """(groups, num_ungrouped): the centered grouping of a CSR graph, one ascending int32 array per
    group, and the number of markers that ended in no group."""
    lib = load_library()
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    nb = np.ascontiguousarray(neighbours, dtype=np.int32)
    if nb.size == 0:
        nb = np.zeros(1, np.int32)
    M = off.size - 1
    G, E, U = C.c_int32(), C.c_int64(), C.c_int64()
    p_off, p_nb = off.ctypes.data_as(C.POINTER(C.c_int64)), nb.ctypes.data_as(C.POINTER(C.c_int32))
    _chk(lib.bann_grouping_centered(M, p_off, p_nb, int(min_group_size), C.byref(G), C.byref(E), None, None,
                                    C.byref(U)), "bann_grouping_centered")
    g_off = np.zeros(G.value + 1, np.int64)
    g_mk = np.zeros(max(E.value, 1), np.int32)
    _chk(lib.bann_grouping_centered(M, p_off, p_nb, int(min_group_size), C.byref(G), C.byref(E),
                                    g_off.ctypes.data_as(C.POINTER(C.c_int64)),
                                    g_mk.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(U)), "bann_grouping_centered")
    return [g_mk[g_off[g]:g_off[g + 1]].copy() for g in range(G.value)], U.value


def write_grouping(path: str, groups) -> None:
    """one "marker<TAB>group" line per member, group by group (read_grouping reads it back)."""
    off, mk = _csr([np.asarray(g, dtype=np.int32) for g in groups])
    _chk(load_library().bann_grouping_write(path.encode(), len(groups), off.ctypes.data_as(C.POINTER(C.c_int64)),
                                            mk.ctypes.data_as(C.POINTER(C.c_int32))), f"bann_grouping_write({path})")


def group_by_ld(ctx, window: int, r2_min: float, min_group_size: int, bim: str = None, max_bp: int = 0,
                missing: str = "zero"):
    """rs-bann group-by-ld on the context's resident cohort: the LD graph from the device (r2 >= r2_min
    within window markers; with a .bim also one chromosome and, for max_bp > 0, at most max_bp apart),
    then the centered grouping.  Returns (groups, num_ungrouped).
    missing: "zero" counts a missing call as genotype 0, as the image stores it; "pairwise" leaves a
    pair's missing individuals out of that pair's r2, as PLINK does (the context needs keep_missing()
    before its .bed load)."""
    if missing not in ("zero", "pairwise"):
        raise ValueError('missing is "zero" or "pairwise"')
    chrom = bp = None
    if bim is not None:
        chrom, bp = read_bim(bim)
    off, nb = ctx.ld_graph(window, r2_min, chrom, bp, max_bp, pairwise=missing == "pairwise")
    return centered_grouping(off, nb, min_group_size)


def encode_bed_payload(g) -> bytes:
    """int8 [M][n] genotypes in {0,1,2}, -1 for a missing call -> the variant-major .bed payload
    (no signature): ceil(n/4) bytes per marker, individual 4q+p in bits 2p of byte q, 2 -> 00, 1 -> 10,
    0 -> 11, -1 -> 01, padding bits 0.  The inverse of the load LUT for the three called values."""
    a = np.asarray(g)
    if a.ndim != 2:
        raise ValueError("genotypes are [num_markers][n]")
    if a.size and (a.min() < -1 or a.max() > 2):
        raise ValueError("genotypes are 0, 1, 2 or -1 (missing)")
    M, n = a.shape
    code = np.array([1, 3, 2, 0], np.uint8)[a.astype(np.int64) + 1]  # index -1 .. 2 -> 01, 11, 10, 00
    padded = np.zeros((M, (n + 3) // 4 * 4), np.uint8)
    padded[:, :n] = code
    q = padded.reshape(M, -1, 4)
    return (q[:, :, 0] | (q[:, :, 1] << 2) | (q[:, :, 2] << 4) | (q[:, :, 3] << 6)).astype(np.uint8).tobytes()


def read_fam(path: str):
    """(lines, count) of a .fam file: one line per individual, kept verbatim (line ends included)."""
    with open(path, "rb") as f:
        lines = f.read().splitlines(keepends=True)
    return lines, len(lines)


def split_indices(n: int, test_n: int, seed: int):
    """(train_idx, test_idx), int64 and ascending (the file order plink --keep keeps): test_n of the n
    individuals drawn without replacement by numpy's default_rng(seed), the others train."""
    n, test_n = int(n), int(test_n)
    if not 0 < test_n < n:
        raise ValueError("test_n must leave both sets non-empty: 0 < test_n < n")
    test = np.sort(np.random.default_rng(seed).choice(n, size=test_n, replace=False)).astype(np.int64)
    mask = np.ones(n, bool)
    mask[test] = False
    return np.flatnonzero(mask).astype(np.int64), test


def kfold_indices(n: int, k: int, seed: int):
    """k disjoint ascending int64 test lists that cover range(n), sizes within 1 of each other: a
    default_rng(seed) permutation cut into k pieces (the train list of fold f is the others' union)."""
    n, k = int(n), int(k)
    if k < 2 or k > n:
        raise ValueError("kfold_indices needs 2 <= k <= n")
    perm = np.random.default_rng(seed).permutation(n)
    return [np.sort(part).astype(np.int64) for part in np.array_split(perm, k)]


def split_train_test(stem: str, test_n: int, seed: int = 0, out_train: str = None, out_test: str = None,
                     phen: str = None, keep_missing: bool = True):
    """scripts/split_train_test.sh without PLINK: stem.bed is loaded once, the train and the test cohort
    are two device subsets of it, and each is written as .bed + .dims with its .fam lines (file order)
    and a copy of the .bim; out stems default to {stem}_train / {stem}_test.  phen: a .phen of the whole
    cohort, written as {out}.phen for each part.  keep_missing: missing calls survive as 01 (off: they
    are written as 11, homozygous A2).  Returns (train_idx, test_idx)."""
    from .context import BannContext
    stem = os.fspath(stem)
    out_train = stem + "_train" if out_train is None else os.fspath(out_train)
    out_test = stem + "_test" if out_test is None else os.fspath(out_test)
    fam, n = read_fam(stem + ".fam")
    train_idx, test_idx = split_indices(n, test_n, seed)
    y = None if phen is None else read_phen(os.fspath(phen))
    if y is not None and y.size != n:
        raise ValueError(f"{phen} has {y.size} phenotypes, {stem}.fam {n} individuals")
    with BannContext(0) as src:
        if keep_missing:
            src.keep_missing(True)
        src.load_bed(stem)
        if src.n != n:
            raise ValueError(f"{stem}: the dims announce {src.n} individuals, the .fam has {n}")
        for out, idx in ((out_train, train_idx), (out_test, test_idx)):
            with src.subset(individuals=idx) as part:
                part.save_bed(out)
            with open(out + ".fam", "wb") as f:
                f.writelines(fam[i] for i in idx)
            shutil.copyfile(stem + ".bim", out + ".bim")
            if y is not None:
                write_phen(out + ".phen", y[idx])
    return train_idx, test_idx


def fill_missing_a2(stem: str, out_stem: str) -> None:
    """scripts/fill_missing_a2.sh without PLINK: stem.bed with every missing call (01) written as
    homozygous A2 (11) into out_stem.bed + .dims, the .fam and the .bim copied."""
    from .context import BannContext
    stem, out_stem = os.fspath(stem), os.fspath(out_stem)
    with BannContext(0) as ctx:
        ctx.keep_missing(True)
        ctx.load_bed(stem)
        ctx.fill_missing_a2()
        ctx.save_bed(out_stem)
    for ext in (".fam", ".bim"):
        shutil.copyfile(stem + ext, out_stem + ext)


def read_phen(path: str) -> np.ndarray:
    lib = load_library()
    n = C.c_int64()
    _chk(lib.bann_phen_read(path.encode(), C.byref(n), None), f"bann_phen_read({path})")
    y = np.zeros(n.value, np.float32)
    _chk(lib.bann_phen_read(path.encode(), C.byref(n), y.ctypes.data_as(C.POINTER(C.c_float))),
         f"bann_phen_read({path})")
    return y


def write_phen(path: str, y) -> None:
    ya = np.ascontiguousarray(y, dtype=np.float32)
    _chk(load_library().bann_phen_write(path.encode(), ya.ctypes.data_as(C.POINTER(C.c_float)), ya.size),
         f"bann_phen_write({path})")


def list_model_files(model_dir: str) -> List[str]:
    """every regular file of model_dir, sorted as Rust sorts the paths (byte order), subdirectories
    skipped (rs-bann.rs:291-297)."""
    d = os.fsencode(model_dir)
    names = sorted(e for e in os.listdir(d) if os.path.isfile(os.path.join(d, e)))
    return [os.fsdecode(os.path.join(d, e)) for e in names]


def format_f32(x) -> str:
    """Rust's f32::to_string: the shortest digits that round-trip, never an exponent; NaN, inf, -inf."""
    v = np.float32(x)
    if np.isnan(v):
        return "NaN"
    if np.isinf(v):
        return "inf" if v > 0 else "-inf"
    return np.format_float_positional(v, unique=True, trim="-")


def write_predictions_csv(file, rows) -> None:
    """one record per model (row), comma separated, newline terminated, values as f32::to_string
    (rs-bann.rs:308-309).  file: a text file object."""
    for row in np.atleast_2d(np.asarray(rows, dtype=np.float32)):
        file.write(",".join(format_f32(v) for v in row) + "\n")


def write_branch_r2_csv(file, rows) -> None:
    """one record per model: the branch r2 values, comma separated, newline terminated, values as
    f32::to_string (the reference prints both this and the predictions with e.to_string()).
    file: a text file object."""
    write_predictions_csv(file, rows)


def write_population_effect_sizes_json(path, values) -> None:
    """the population effect sizes as one flat JSON array of numbers, each the shortest decimal that
    parses back to the same f32.  Byte-equality with serde_json's float formatting is NOT claimed
    (it switches to exponents where this writer keeps positional digits); the parsed values are
    identical.  JSON has no NaN or infinity: a non-finite value raises ValueError and nothing is written."""
    v = np.asarray(values, dtype=np.float32).ravel()
    if not np.all(np.isfinite(v)):
        raise ValueError("non-finite population effect size: not representable in JSON")
    # "-0" would parse as the integer 0 and lose its sign: every number carries a fraction part
    text = "[" + ",".join(t if "." in t else t + ".0" for t in map(format_f32, v)) + "]"
    json.loads(text)  # well-formed by construction; a cheap guard against a formatting slip
    with open(path, "w") as f:
        f.write(text)
