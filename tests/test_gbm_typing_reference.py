"""The reference typing (SMC_MATH_REF: rows_ref_kernel) and the f64 engine of csrc/gbm.hip against the independent
reference of tests/helpers/gbm_reference.py, on the CPU.

Reference typing: the oracle's kernel mode with MATH_REF (which tests/test_gpu_reference_math.py shows equal to
rows_ref_kernel + cf_kernel bit for bit in portable math) stands in for the kernel; every stored path element, row sum
and target bin has to lie within the bound of gbm_reference.REF_PORTABLE.

f64 engine: oracle.gbm_paths, oracle.normals and oracle.training_targets with dtype="float64" (today's yardstick of
every Real = double kernel, whose normals are the C restatement of the kernel's own table-driven math) are held to a
long-double statement of the model within the bound of gbm_reference.F64_ENGINE, and that bound is shown to lie
below the project's float64 tolerance on every case row, so the new check is never the looser one.
tests/test_gpu_gbm_typing_reference.py holds the kernels themselves to the same references.

The sensitivity tests give the bounds their meaning: each wrong reading listed there, put in the reference's place,
has to leave the bound somewhere on the case set, and so do the f32 engine's paths put in the reference typing's."""

from __future__ import annotations

import functools

import numpy as np
import pytest

from tests.helpers import ATOL_FLOAT64, RTOL_FLOAT64
from tests.helpers import gbm_reference as gref
from tests.test_gbm_reference import (
    FLAT,
    MUTANT_CASES,
    ORD0,
    SEED,
    SHAPE,
    WRONG_NORMALS,
    WRONG_OUTPUTS,
    WRONG_PATHS,
    WRONG_WORDS,
    _oracle,
    _wrong_paths,
    case_rows,
)

GRID_T = [1, 2, 3, 5, 16, 17, 40]
GRID_P = [21, 528, 693, 1024, 4096]
SCHEMES = {gref.LOG_EULER: "log Euler", gref.SIMPLE_EULER: "simple Euler"}
needs_longdouble = pytest.mark.skipif(not gref.LONGDOUBLE_OK, reason="numpy.longdouble has no 64-bit significand here")


def _reference(ty: gref.Typing, T: int, P: int, scheme: int, normalize: bool, *, words: dict | None = None,
               normals: dict | None = None, paths: dict | None = None, outputs: dict | None = None,
               z_scale: float = 1.0) -> tuple[gref.GbmRef, np.ndarray, np.ndarray]:
    """(the reference of the case rows in the typing ty, its normals z, their radii); the dicts carry wrong readings."""
    rows, _ = case_rows(scheme, normalize)
    N, M = SHAPE[P]
    w = gref.stream_words(_oracle(), rows.shape[0], T, P, SEED, ORD0, **(words or {}))
    kind = {"f64": True, "longdouble": True} if ty.f64_normals else {}
    z, rad = gref.normals(w, T, P, **({**kind, **normals} if normals is not None else kind))
    x, dx = gref.paths(rows, T, z * z_scale, rad, ty, scheme, **(paths or {}))
    ref = gref.outputs(rows, x, dx, N=N, M=M, normalize=normalize, keep_paths=True, fmt=ty.fmt, **(outputs or {}))
    return ref, z, rad


def shares(got: dict[str, np.ndarray], ref: gref.GbmRef, bounds: gref.GbmRef | None = None) -> dict[str, float]:
    b = ref if bounds is None else bounds
    return {"paths": gref.share_used(got["paths"], ref.x, b.dx),
            "row sums": gref.share_used(got["row sums"], ref.rowsum, b.rowsum_bound),
            "targets": gref.complex_share_used(got["targets"], ref.targets, b.targets_bound)}


LARGEST: dict[tuple[str, str, str], float] = {}  # (typing, scheme, kind) -> the largest share the sweeps have seen


def _note(typing: str, scheme: int, used: dict[str, float]) -> None:
    for kind, v in used.items():
        key = (typing, SCHEMES[scheme], kind)
        LARGEST[key] = max(LARGEST.get(key, 0.0), v)


def _largest(typing: str) -> str:
    return ", ".join(f"{s} {k} {v:.3f}" for (ty, s, k), v in sorted(LARGEST.items()) if ty == typing)


# ---- reference typing, portable normals ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def _ref_kernel_mode(T: int, P: int, scheme: int, normalize: bool, flag: bool = True) -> dict[str, np.ndarray]:
    """The oracle's kernel mode with MATH_REF (flag = False: the f32 engine's own typing)."""
    oracle = _oracle()
    rows, _ = case_rows(scheme, normalize)
    N, M = SHAPE[P]
    s = scheme | (oracle.MATH_REF if flag else 0)
    kp, _, krs = oracle.kernel_paths(rows, T, P, SEED, ORD0, s, want_paths=True)
    kt, _ = oracle.kernel_targets(rows, T, N, M, SEED, ORD0, s, normalize)
    return {"paths": kp, "row sums": krs, "targets": kt}


@pytest.mark.parametrize("P", GRID_P)
@pytest.mark.parametrize("T", GRID_T)
def test_reference_typing_kernel_mode_within_the_bound(T, P) -> None:
    for scheme in SCHEMES:
        for normalize in (False, True):
            label = f"reference typing T {T} P {P} {SCHEMES[scheme]} {'NORMALIZE' if normalize else 'RAW'}"
            ref, _, _ = _reference(gref.REF_PORTABLE, T, P, scheme, normalize)
            used = shares(_ref_kernel_mode(T, P, scheme, normalize), ref)
            rel = ref.dx[:, -1] / np.abs(ref.x[:, -1])
            print(f"{label}: share of the bound used " + ", ".join(f"{k} {v:.3f}" for k, v in used.items())
                  + f"; last-row path bound {rel.min():.2e} .. {rel.max():.2e} relative")
            _note("reference", scheme, used)
            assert max(used.values()) < 1.0, (label, used)
    print("largest share so far: " + _largest("reference"))


# ---- f64 engine ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def _f64_oracle(T: int, P: int, scheme: int, normalize: bool) -> dict[str, np.ndarray]:
    oracle = _oracle()
    rows, _ = case_rows(scheme, normalize)
    N, M = SHAPE[P]
    paths, _, rowsum = oracle.gbm_paths(rows, T, P, SEED, ORD0, scheme, dtype="float64", want_paths=True)
    tg = oracle.training_targets(rows, T, N, M, SEED, ORD0, scheme, normalize, dtype="float64")
    z = np.stack([oracle.normals(SEED, ORD0 + b, T, P, dtype="float64") for b in range(rows.shape[0])])
    return {"paths": paths, "row sums": rowsum, "targets": tg, "normals": z}


def normal_bound(ty: gref.Typing, z: np.ndarray, rad: np.ndarray) -> np.ndarray:
    """eps_z of the typing (gbm_reference's docstring)."""
    return ty.eps.radius + rad * ty.eps.sincos + ty.nz * ty.uz * np.abs(z)


def assert_below_the_float64_tolerance(ref: gref.GbmRef, label: str) -> None:
    """The derived bound is the tighter check, in the form the project applies its float64 tolerance in
    (tests/test_gpu_engine.py): the stored paths of every case row in that row's norm, every row sum by itself, the
    targets and the price means in the norm of the whole batch; each below RTOL_FLOAT64 |want| + ATOL_FLOAT64.
    No a-priori bound can be below that tolerance element by element: a reflected simple-Euler path may land anywhere
    near 0 with an absolute error, and a target that is exactly 0 (a put that never pays) still carries the roundings
    of x s about the strike summed over N columns, against ATOL_FLOAT64 alone.  The standard errors are left out: their
    bound carries the cancellation of sum v^2 - P m^2 in f64, sqrt(4 P 2^-53 sum v^2 / (P (P - 1))), which no relative
    tolerance of 1e-10 covers."""
    def norm(a: np.ndarray, axis=None) -> np.ndarray:
        return np.linalg.norm(np.abs(a).astype(np.float64), axis=axis)

    B = ref.x.shape[0]
    assert np.all(norm(ref.dx.reshape(B, -1), 1) <= RTOL_FLOAT64 * norm(ref.x.reshape(B, -1), 1) + ATOL_FLOAT64), label
    assert np.all(ref.rowsum_bound <= RTOL_FLOAT64 * np.abs(ref.rowsum) + ATOL_FLOAT64), (label, "row sums")
    assert np.sqrt(2.0) * norm(ref.targets_bound) <= RTOL_FLOAT64 * norm(ref.targets) + ATOL_FLOAT64, (label, "targets")
    assert norm(ref.price_bound[:, :3]) <= RTOL_FLOAT64 * norm(ref.price[:, :3]) + ATOL_FLOAT64, (label, "price means")


@needs_longdouble
@pytest.mark.parametrize("P", GRID_P)
@pytest.mark.parametrize("T", GRID_T)
def test_f64_oracle_within_the_bound(T, P) -> None:
    for scheme in SCHEMES:
        for normalize in (False, True):
            label = f"f64 T {T} P {P} {SCHEMES[scheme]} {'NORMALIZE' if normalize else 'RAW'}"
            ref, z, rad = _reference(gref.F64_ENGINE, T, P, scheme, normalize)
            assert ref.x.dtype == np.longdouble and ref.targets.dtype == np.clongdouble
            assert_below_the_float64_tolerance(ref, label)
            got = _f64_oracle(T, P, scheme, normalize)
            used = shares(got, ref)
            used["normals"] = gref.share_used(got["normals"], z, normal_bound(gref.F64_ENGINE, z, rad))
            rel = (ref.dx[:, -1] / np.abs(ref.x[:, -1])).astype(np.float64)
            print(f"{label}: share of the bound used " + ", ".join(f"{k} {v:.3f}" for k, v in used.items())
                  + f"; last-row path bound {rel.min() * 2.0 ** 53:.1f} .. {rel.max() * 2.0 ** 53:.1f} 2^-53 relative")
            _note("f64", scheme, used)
            assert max(used.values()) < 1.0, (label, used)
    print("largest share so far: " + _largest("f64"))


# ---- sensitivity: wrong readings leave each bound --------------------------------------------------------------------
def _factor(got: dict[str, np.ndarray], wrong: gref.GbmRef, good: gref.GbmRef) -> tuple[float, bool]:
    """(the largest |got - wrong| / good's bound over the contracts but the flat one, whether the flat contract leaves
    its bound): tests/test_gbm_reference._factor, on the outputs these typings have."""
    trios = [(got["paths"], wrong.x, good.dx), (got["row sums"], wrong.rowsum, good.rowsum_bound),
             (got["targets"].real, wrong.targets.real, good.targets_bound),
             (got["targets"].imag, wrong.targets.imag, good.targets_bound)]
    others = np.arange(good.price.shape[0]) != FLAT
    largest = max(gref.share_used(g[others], w[others], b[others]) for g, w, b in trios)
    return largest, max(gref.share_used(g[FLAT], w[FLAT], b[FLAT]) for g, w, b in trios) > 1.0


def _mutant_factors(ty: gref.Typing, kernel_mode, mutants: dict[str, dict]) -> dict[str, float]:
    """name -> the factor by which the wrong reading leaves the bound over MUTANT_CASES (infinity where only the flat
    contract, whose bound is zero or a few ulps, leaves it)."""
    factor = {name: 0.0 for name in mutants}
    zero_hit = {name: False for name in mutants}
    for T, P, scheme, normalize in MUTANT_CASES:
        rows, _ = case_rows(scheme, normalize)
        good, _, _ = _reference(ty, T, P, scheme, normalize)
        got = kernel_mode(T, P, scheme, normalize)
        assert max(shares(got, good).values()) < 1.0, (T, P, scheme, normalize)
        for name, kw in mutants.items():
            if (name, scheme) in (("no -v^2/2", gref.SIMPLE_EULER), ("no reflection", gref.LOG_EULER)):
                continue  # a reading of the other scheme
            kw = {**kw, "paths": {**kw.get("paths", {}), **_wrong_paths(rows, T, scheme, name)}}
            if name == "drift off by 1e-12 per step":
                X0, _, Tm, r, d, v = gref.fields(rows)
                drift = r - d - 0.5 * v * v if scheme == gref.LOG_EULER else r - d
                kw["paths"] = {"drift": drift + 1e-12 / (Tm / T)}
            with np.errstate(all="ignore"):
                wrong, _, _ = _reference(ty, T, P, scheme, normalize, **kw)
                largest, hit = _factor(got, wrong, good)
            factor[name] = max(factor[name], largest)
            zero_hit[name] |= hit
    return {name: v if v > 1.0 or not zero_hit[name] else np.inf for name, v in factor.items()}


def _report(title: str, factor: dict[str, float]) -> None:
    print(f"{title}: factor by which each wrong reading leaves the bound: "
          + ", ".join(f"{k}: {v:.3g}" for k, v in factor.items()))
    print(f"the closest: {min(factor, key=factor.get)}")
    survivors = [k for k, v in factor.items() if not v > 1.0]
    assert not survivors, survivors


# the readings of tests/test_gbm_reference.py that reach the reference typing's outputs (stored paths, row sums and
# targets: the two barrier readings, "strict barrier comparisons" and "X0 monitored", belong to path_price_kernel,
# which has no reference typing), and the state rounded to f32 between steps
REF_MUTANTS: dict[str, dict] = {
    **{k: {"normals": v} for k, v in WRONG_NORMALS.items()}, **{k: {"words": v} for k, v in WRONG_WORDS.items()},
    **{k: {} for k in WRONG_PATHS},
    **{k: {"outputs": v} for k, v in WRONG_OUTPUTS.items() if k not in ("strict barrier comparisons", "X0 monitored")},
    "state rounded to f32 after every step": {"paths": {"round_state": True}},
}


def test_wrong_readings_leave_the_reference_typing_bound() -> None:
    factor = _mutant_factors(gref.REF_PORTABLE, _ref_kernel_mode, REF_MUTANTS)
    assert len(factor) == 12
    _report("reference typing", factor)


def test_unscaled_hardware_normals_leave_the_reference_hw_bound() -> None:
    """SMC_MATH_REF | SMC_MATH_HW: normal_pair<true> returns z / sqrt(2 ln 2) and lane_rows_ref rescales it.  The
    hardware normals cannot be restated on a CPU; the portable MATH_REF kernel mode lies within the wider REF_HW bound
    as well, and a reference whose normals are left unscaled leaves that bound."""
    worst = 0.0
    for T, P, scheme, normalize in MUTANT_CASES:
        good, _, _ = _reference(gref.REF_HW, T, P, scheme, normalize)
        got = _ref_kernel_mode(T, P, scheme, normalize)
        assert max(shares(got, good).values()) < 1.0, (T, P, scheme, normalize)
        wrong, _, _ = _reference(gref.REF_HW, T, P, scheme, normalize, z_scale=1.0 / gref.NORMAL_SCALE)
        worst = max(worst, _factor(got, wrong, good)[0])
    print(f"reference_hw, normals left unscaled by sqrt(2 ln 2): factor {worst:.3g}")
    assert worst > 1.0


def test_f32_engine_paths_leave_the_reference_typing_bound() -> None:
    """The f32 engine's stored paths (kernel mode without MATH_REF) in place of the reference typing's: the bound tells
    the two typings apart from T = 5 on; at T <= 2 a path is one or two f32 steps from X0 and both typings sit within a
    few f32 roundings of the model, so the factor there is printed and not asserted."""
    factor = {}
    for T, P in ((1, 1024), (2, 1024), (5, 693), (16, 4096), (40, 528)):
        good, _, _ = _reference(gref.REF_PORTABLE, T, P, gref.LOG_EULER, True)
        f32 = _ref_kernel_mode(T, P, gref.LOG_EULER, True, False)
        share = np.abs(f32["paths"] - good.x) / good.dx
        per_row = share.reshape(share.shape[0], -1).max(axis=1)
        factor[(T, P)] = float(per_row.max())
        print(f"f32 engine's paths against the reference typing's bound at T {T} P {P}: factor {per_row.max():.3g}, "
              f"{int((per_row > 1.0).sum())} of {per_row.size} case rows leave it")
    separating = [T for (T, _), v in factor.items() if v > 1.0]
    print(f"the smallest T that separates the typings: {min(separating)}")
    assert all(factor[c] > 1.0 for c in ((5, 693), (16, 4096), (40, 528))), factor


F64_MUTANTS: dict[str, dict] = {
    "f32 uniforms (a >> 9) 2^-23": {"normals": {"f64": False, "longdouble": False}},
    "plain 32-bit angle b 2^-32": {"normals": {"plain_angle": True}},
    "cosine and sine exchanged": {"normals": {"exchange": True}},
    "tail pair k to paths k, k + 2": {"normals": {"tail_stride": True}},
    "no stream span": {"words": {"span": False}},
    "drift off by 1e-12 per step": {},
    "dt = T / (steps + 1)": {},
}


@needs_longdouble
def test_wrong_readings_leave_the_f64_bound() -> None:
    factor = _mutant_factors(gref.F64_ENGINE, _f64_oracle, F64_MUTANTS)
    assert len(factor) == 7
    _report("f64 engine", factor)
