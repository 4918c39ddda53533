"""The single-asset GBM engine against the independent float64 reference of tests/helpers/gbm_reference.py, on the
CPU: the oracle's kernel mode (oracle.kernel_paths / kernel_targets, which tests/test_gpu_engine.py shows equal to the
kernels bit for bit in portable math) and the portable restatements of the two pricing blocks
(tests/helpers/gbm_restate.py, held bit for bit by tests/test_gpu_price.py and tests/test_gpu_path_price.py) stand in
for the kernels, and every stored path element, row sum, target bin and price column has to lie within the a-priori
bound the helper derives.  tests/test_gpu_gbm_reference.py holds the kernels themselves to the same reference, in
portable and in SMC_MATH_HW math.

The sensitivity test is what gives the bound its meaning: each wrong reading of the engine listed there, put in the
reference's place, has to leave the bound somewhere on the case set."""

from __future__ import annotations

import functools

import numpy as np
import pytest

from tests.helpers import gbm_reference as gref
from tests.helpers import gbm_restate as gr
from tests.helpers import make_domain_bounds

SEED = 7
ORD0 = 3
N_SOBOL = 3
# P -> (N, M) of the training call
SHAPE = {21: (7, 3), 528: (16, 33), 693: (99, 7), 1024: (64, 16), 1030: (10, 103), 2048: (64, 32), 4096: (64, 64)}
REST = [c for c in range(20) if c != 17]  # the columns of smc_gbm_price_paths but the knocked share


def _oracle():
    import oracle  # noqa: PLC0415

    oracle.build()
    return oracle


@functools.lru_cache(maxsize=None)
def case_rows(scheme: int, normalize: bool) -> tuple[np.ndarray, np.ndarray]:
    """(contract rows [12, 6], barriers [12, 2]) of every case: Sobol-drawn rows in the default bounds with the
    default barriers, then the hand-built rows with theirs.  tests/test_gpu_gbm_reference.py uses the same."""
    lo, hi = make_domain_bounds().arrays()
    sobol = _oracle().sobol_contracts(SEED, 0, N_SOBOL, lo, hi)
    rows = np.concatenate([sobol, gref.hand_built_rows()])
    bars = np.concatenate([gref.default_barriers(sobol), gref.hand_built_barriers(scheme, normalize)])
    rows.setflags(write=False)
    bars.setflags(write=False)
    return rows, bars


@functools.lru_cache(maxsize=8)
def _kernel_mode(T: int, P: int, scheme: int, normalize: bool) -> dict[str, np.ndarray]:
    """What the portable kernels give, restated on the CPU."""
    oracle = _oracle()
    rows, bars = case_rows(scheme, normalize)
    N, M = SHAPE[P]
    kp, _, krs = oracle.kernel_paths(rows, T, P, SEED, ORD0, scheme, want_paths=True)
    kt, _ = oracle.kernel_targets(rows, T, N, M, SEED, ORD0, scheme, normalize)
    return {"paths": kp, "row sums": krs, "targets": kt,
            "price": gr.price_f32(oracle, rows, T, P, SEED, ORD0, scheme, int(normalize))["cols"],
            "path price": gr.path_price_f32(oracle, rows, bars, T, P, SEED, ORD0, scheme, int(normalize))["cols"]}


def _wrong_paths(rows: np.ndarray, T: int, scheme: int, wrong: str) -> dict:
    X0, _, Tm, r, d, v = gref.fields(rows)
    drift = r - d - 0.5 * v * v if scheme == gref.LOG_EULER else r - d
    return {"no -v^2/2": {"drift": r - d}, "drift off by 1e-6 per step": {"drift": drift + 1e-6 / (Tm / T)},
            "dt = T / (steps + 1)": {"dt": Tm / (T + 1)}, "no reflection": {"reflect": False}}.get(wrong, {})


WRONG_WORDS = {"no stream span": {"span": False}}
WRONG_NORMALS = {"cosine and sine exchanged": {"exchange": True}, "tail pair k to paths k, k + 2": {"tail_stride": True},
                 "u1 without the complement": {"complement": False}}
WRONG_OUTPUTS = {"forward of row t at t dt": {"early": True}, "(M, N) reshape transposed": {"transposed": True},
                 "strict barrier comparisons": {"strict": True}, "X0 monitored": {"with_x0": True},
                 "discount e^{-(r - d) T}": {"carry": True}}
WRONG_PATHS = ("no -v^2/2", "drift off by 1e-6 per step", "dt = T / (steps + 1)", "no reflection")
MUTANTS = (*WRONG_NORMALS, *WRONG_WORDS, *WRONG_PATHS, *WRONG_OUTPUTS)


def _reference(T: int, P: int, scheme: int, normalize: bool, wrong: str = "") -> gref.GbmRef:
    oracle = _oracle()
    rows, bars = case_rows(scheme, normalize)
    N, M = SHAPE[P]
    words = gref.stream_words(oracle, rows.shape[0], T, P, SEED, ORD0, **WRONG_WORDS.get(wrong, {}))
    z, rad = gref.normals(words, T, P, **WRONG_NORMALS.get(wrong, {}))
    x, dx = gref.paths(rows, T, z, rad, gref.PORTABLE, scheme, **_wrong_paths(rows, T, scheme, wrong))
    return gref.outputs(rows, x, dx, N=N, M=M, normalize=normalize, bars=bars, keep_paths=True,
                        **WRONG_OUTPUTS.get(wrong, {}))


def shares(got: dict[str, np.ndarray], ref: gref.GbmRef, bounds: gref.GbmRef | None = None) -> dict[str, float]:
    """The largest share of the bound used per output kind: got's values against ref's, by the bounds of `bounds`."""
    b = ref if bounds is None else bounds
    return {"paths": gref.share_used(got["paths"], ref.x, b.dx),
            "row sums": gref.share_used(got["row sums"], ref.rowsum, b.rowsum_bound),
            "targets": gref.complex_share_used(got["targets"], ref.targets, b.targets_bound),
            "price": gref.share_used(got["price"], ref.price, b.price_bound),
            "path price": gref.share_used(got["path price"][:, REST], ref.path[:, REST], b.path_bound[:, REST]),
            "knocked share": gref.share_used(got["path price"][:, 17], ref.path[:, 17], b.path_bound[:, 17])}


def assert_within(used: dict[str, float], label: str) -> None:
    """Every kind strictly inside its bound; the knocked share is a count and may use its whole tolerance."""
    assert used["knocked share"] <= 1.0, (label, used)
    assert max(v for k, v in used.items() if k != "knocked share") < 1.0, (label, used)


# ---- the sweep -------------------------------------------------------------------------------------------------------
LARGEST: dict[tuple[str, str], float] = {}  # (scheme, output kind) -> the largest share the sweep has seen so far


@pytest.mark.parametrize("P", [21, 528, 693, 1024, 2048, 4096])
@pytest.mark.parametrize("T", [1, 2, 3, 5, 16, 17, 40])
def test_kernel_mode_within_the_bound(T, P) -> None:
    for scheme in (gref.LOG_EULER, gref.SIMPLE_EULER):
        for normalize in (False, True):
            label = f"T {T} P {P} {'log' if scheme == gref.LOG_EULER else 'simple'} Euler {'NORMALIZE' if normalize else 'RAW'}"
            ref = _reference(T, P, scheme, normalize)
            assert gref.count_ok(ref.doubt, P), (label, ref.doubt)
            used = shares(_kernel_mode(T, P, scheme, normalize), ref)
            rel = ref.dx[:, -1] / np.abs(ref.x[:, -1])
            print(f"{label}: share of the bound used " + ", ".join(f"{k} {v:.3f}" for k, v in used.items())
                  + f"; last-row path bound {rel.min():.2e} .. {np.median(rel):.2e} relative")
            for kind, v in used.items():
                key = ("log Euler" if scheme == gref.LOG_EULER else "simple Euler", kind)
                LARGEST[key] = max(LARGEST.get(key, 0.0), v)
            assert_within(used, label)
    print("largest share so far: " + ", ".join(f"{s} {k} {v:.3f}" for (s, k), v in sorted(LARGEST.items())))


# ---- sensitivity: wrong readings leave the bound ---------------------------------------------------------------------
# (T, P, scheme, normalize): an even T in two chunks, an odd T with a ragged P, the stream span, the flat contract's
# barrier (simple Euler, RAW), a second odd T in log-Euler
MUTANT_CASES = [(16, 4096, 0, True), (5, 693, 1, True), (2, 1024, 0, False), (3, 2048, 1, False), (7, 1030, 0, True)]


FLAT = N_SOBOL + list(gref.HAND_BUILT).index("flat")


def _factor(got: dict[str, np.ndarray], wrong: gref.GbmRef, good: gref.GbmRef) -> tuple[float, bool]:
    """(the largest |got - wrong| / good's bound over the contracts but the flat one and the columns but the knocked
    share, whether the flat contract or a knocked share leaves its bound).  The flat contract's bounds are zero or a
    few ulps of f64 and the knocked share's tolerance is mostly zero: they would turn nearly every factor into infinity
    or 1e6, which says nothing about the other elements, so they speak only where nothing else does."""
    trios = [(got["paths"], wrong.x, good.dx), (got["row sums"], wrong.rowsum, good.rowsum_bound),
             (got["targets"].real, wrong.targets.real, good.targets_bound),
             (got["targets"].imag, wrong.targets.imag, good.targets_bound),
             (got["price"], wrong.price, good.price_bound),
             (got["path price"][:, REST], wrong.path[:, REST], good.path_bound[:, REST])]
    others = np.arange(good.price.shape[0]) != FLAT
    largest = max(gref.share_used(g[others], w[others], b[others]) for g, w, b in trios)
    flat = max(gref.share_used(g[FLAT], w[FLAT], b[FLAT]) for g, w, b in trios)
    count = gref.share_used(got["path price"][:, 17], wrong.path[:, 17], good.path_bound[:, 17])
    return largest, flat > 1.0 or count > 1.0


@functools.lru_cache(maxsize=None)
def _mutant_factors() -> dict[str, float]:
    """name -> the factor by which the wrong reading leaves the bound, over the case set: the largest over the
    elements of _factor where that exceeds 1, else infinity if the flat contract or a knocked share leaves its bound."""
    factor = {name: 0.0 for name in MUTANTS}
    zero_hit = {name: False for name in MUTANTS}
    for T, P, scheme, normalize in MUTANT_CASES:
        good = _reference(T, P, scheme, normalize)
        got = _kernel_mode(T, P, scheme, normalize)
        assert_within(shares(got, good), (T, P, scheme, normalize))
        for name in MUTANTS:
            if name == "no -v^2/2" and scheme != gref.LOG_EULER or name == "no reflection" and scheme != gref.SIMPLE_EULER:
                continue
            with np.errstate(all="ignore"):
                wrong = _reference(T, P, scheme, normalize, name)
                largest, hit = _factor(got, wrong, good)
                factor[name] = max(factor[name], largest)
                zero_hit[name] |= hit
    return {name: v if v > 1.0 or not zero_hit[name] else np.inf for name, v in factor.items()}


def test_wrong_readings_leave_the_bound() -> None:
    factor = _mutant_factors()
    print("factor by which each wrong reading leaves the bound: " + ", ".join(f"{k}: {v:.3g}" for k, v in factor.items()))
    print(f"the closest: {min(factor, key=factor.get)}")
    assert len(factor) == 13
    survivors = [k for k, v in factor.items() if not v > 1.0]
    assert not survivors, survivors


# ---- wrong readings of the cells the instantiation ledger added ------------------------------------------------------
# What an instantiation of tests/helpers/instantiations.py could do wrong that the thirteen readings above do not say:
# * resident_kernel<.., ONTHEFLY> is the RAW kernel (pay_raw(.., 1.0)): it must not apply NORMALIZE's scale;
# * a STORE_TERMINAL instantiation hands out one row: it must be row T - 1, not T - 2;
# * the paths_kernel of ragged shapes keeps the f64 terminal sum behind one padding element where P is odd: the lane
#   that straddles P simulates path P as well (its draws are made and dropped) and must not add it to the sum.
# Each is put in the reference's place for the outputs it touches alone, against the unchanged bound, contract by
# contract.  The condition: in every case where the reading applies it leaves the bound, and the first two do so on
# every contract but the flat one (whose bounds are zero) and, for the reading that shows in the targets only, but
# those whose reference put is zero on every path (their target is zero under either reading: nothing is there to
# see).  The third adds one path to a sum of P: that is visible where the path is larger than the sum's bound, which
# it is for the contracts of moderate volatility (factors of 10 to 3000) and is not for those with v sqrt(T) of 3 and
# more, where a typical path is a vanishing part of a sum that a few large ones carry (factors down to 0.03).  The
# test prints on how many contracts each reading shows.
CELL_MUTANTS = ("RAW targets on the NORMALIZE scale", "terminal row taken as row T - 2",
                "odd-P padding element in the terminal sum")
CELL_CASES = [*MUTANT_CASES, (7, 693, 0, True)]  # and the ragged split pair's own shape, in log-Euler


def _per_contract(got: np.ndarray, want: np.ndarray, bound: np.ndarray) -> np.ndarray:
    """[B]: the largest |got - want| / bound of each contract (complex: of the real and the imaginary parts)."""
    if np.iscomplexobj(want):
        return np.maximum(_per_contract(got.real, want.real, bound), _per_contract(got.imag, want.imag, bound))
    B = want.shape[0]
    return np.array([gref.share_used(got[b], want[b], bound[b]) for b in range(B)])


def _targets_given_sum(rows: np.ndarray, good: gref.GbmRef, tot: np.ndarray, T: int, N: int, M: int) -> np.ndarray:
    """NORMALIZE targets of the reference's terminal row scaled by F_T / (tot / P)."""
    F, eF = gref.forwards(rows, T)
    xs, dxs = gref.scaled(good.xT, good.dxT, tot, good.rowsum_bound[:, -1], F[:, -1], eF[:, -1])
    df, edf = gref.discount(rows)
    put, dput = gref.payoff(1.0, gref.fields(rows)[1][:, None], xs, dxs, df[:, None], edf[:, None])
    return gref.targets(put, dput, N, M)[0]


@functools.lru_cache(maxsize=None)
def _cell_mutant_factors() -> dict[str, dict[tuple, np.ndarray]]:
    """reading -> case -> [B] factor by which it leaves the bound per contract (NaN: the contract cannot show it)."""
    oracle = _oracle()
    out: dict[str, dict[tuple, np.ndarray]] = {name: {} for name in CELL_MUTANTS}
    for case in CELL_CASES:
        T, P, scheme, normalize = case
        N, M = SHAPE[P]
        rows, _ = case_rows(scheme, normalize)
        good = _reference(T, P, scheme, normalize)
        got = _kernel_mode(T, P, scheme, normalize)
        assert_within(shares(got, good), case)
        K = gref.fields(rows)[1]
        flat = np.arange(rows.shape[0]) == FLAT
        if not normalize:
            scale = good.xT.shape[-1] * gref.forwards(rows, T)[0][:, -1] / good.rowsum[:, -1]  # F_T / mean x_T
            blind = flat | np.all(np.maximum(K[:, None] - good.xT, 0.0) == 0.0, axis=1) \
                | np.all(np.maximum(K[:, None] - good.xT * scale[:, None], 0.0) == 0.0, axis=1)
            wrong = _targets_given_sum(rows, good, good.rowsum[:, -1], T, N, M)
            f = _per_contract(got["targets"], wrong, good.targets_bound)
            out[CELL_MUTANTS[0]][case] = np.where(blind, np.nan, f)
        if T >= 2:
            f = _per_contract(got["paths"][:, -1], good.x[:, T - 2], good.dxT)
            out[CELL_MUTANTS[1]][case] = np.where(flat, np.nan, f)
        if P % 2 and T >= 3:
            words = gref.stream_words(oracle, rows.shape[0], T, P + 1, SEED, ORD0)
            assert words.shape[1] == -(-P // 4)  # path P belongs to the last group of the P paths
            z, rad = gref.normals(words, T, P + 1)
            x1, _ = gref.paths(rows, T, z, rad, gref.PORTABLE, scheme)
            np.testing.assert_array_equal(x1[:, :, :P], good.x)
            tot = good.rowsum[:, -1] + x1[:, -1, P]
            f = _per_contract(got["row sums"][:, -1], tot, good.rowsum_bound[:, -1])
            if normalize:
                wrong = _targets_given_sum(rows, good, tot, T, N, M)
                f = np.maximum(f, _per_contract(got["targets"], wrong, good.targets_bound))
            out[CELL_MUTANTS[2]][case] = np.where(flat, np.nan, f)
    return out


def test_wrong_readings_of_the_new_cells_leave_the_bound() -> None:
    factors = _cell_mutant_factors()
    for name in CELL_MUTANTS:
        cases = factors[name]
        assert cases, name
        seen = np.concatenate(list(cases.values()))
        print(f"{name}: over {len(cases)} cases, the factor by which it leaves the bound per contract "
              f"{np.nanmin(seen):.3g} .. {np.nanmax(seen):.3g}; contracts that cannot show it "
              f"{sorted({int(b) for f in cases.values() for b in np.flatnonzero(np.isnan(f))})}")
        for case, f in cases.items():
            able = f[~np.isnan(f)]
            assert able.size >= 8, (name, case)  # the exemptions stay exceptions
            print(f"  {case}: leaves the bound on {int(np.sum(able > 1.0))} of {able.size} contracts, "
                  f"factor {able.min():.3g} .. {able.max():.3g}")
            assert able.max() > 1.0, (name, case, f.tolist())  # in every case, not only somewhere on the case set
            if name != CELL_MUTANTS[2]:
                assert np.all(able > 1.0), (name, case, f.tolist())


# ---- the reference against closed forms of its own -------------------------------------------------------------------
def test_reference_put_is_blacks_put(oracle) -> None:
    rows = gr.contracts(8)
    ref = gref.reference(oracle, rows, 16, 65536, SEED, 0)
    black = np.array([oracle.black_put(*c) for c in rows.tolist()])
    zs = np.abs(ref.price[:, 0] - black) / ref.price[:, 3]
    print(f"|put - Black| / stderr: {np.round(zs, 2).tolist()}")
    assert np.all(ref.price[:, 0] > 0.0) and np.all(zs <= 4.0)
    F = rows[:, 0] * np.exp((rows[:, 3] - rows[:, 4]) * rows[:, 2])
    np.testing.assert_allclose(ref.price[:, 2], F, rtol=1e-12)  # NORMALIZE puts the mean on the forward
    parity = ref.price[:, 1] - ref.price[:, 0] - np.exp(-rows[:, 3] * rows[:, 2]) * (F - rows[:, 1])
    assert np.max(np.abs(parity) / rows[:, 1]) < 1e-12


def test_reference_normals_are_standard(oracle) -> None:
    for T in (1, 2, 5):
        z, rad = gref.normals(gref.stream_words(oracle, 1, T, 65536, SEED, ORD0), T, 65536)
        tol = 4.0 / np.sqrt(65536)
        assert np.all(np.abs(z.mean(axis=2)) <= tol) and np.all(np.abs(z.var(axis=2) - 1.0) <= 2 * tol), T
        assert np.all(np.abs(z) <= rad)
        if T > 1:
            assert np.all(np.abs(np.corrcoef(z[0]) - np.eye(T)) <= tol), T


def test_path_columns_tie_to_the_price_columns(oracle) -> None:
    rows = gr.contracts(4)
    ref = gref.reference(oracle, rows, 1, 528, SEED, ORD0, bars=gr.barriers(rows))
    np.testing.assert_array_equal(ref.path[:, [6, 7, 14, 15]], ref.price[:, [0, 1, 3, 4]])
    # one monitoring date: the average, the maximum and the minimum are the terminal value
    np.testing.assert_allclose(ref.path[:, [0, 1, 4, 5]], ref.path[:, [6, 7, 6, 7]], rtol=1e-14)
    free = gref.reference(oracle, rows, 1, 528, SEED, ORD0, bars=np.array([[0.0, np.inf]] * 4))
    assert np.all(free.path[:, 17] == 0.0) and np.all(free.doubt == 0)
    np.testing.assert_array_equal(free.path[:, [2, 3]], free.path[:, [6, 7]])
