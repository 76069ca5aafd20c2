"""The dense fill's operand stage (option dense_stage): with the stage, an entry's record and phase
blocks are copied into LDS one entry ahead and read from there; without it every entry loads its own.  Only where the
operands come from differs, so everything a caller can see must be equal BYTE FOR BYTE: matrices, interval counts,
return codes, deferred integrals, and a whole root search with its iterates."""
import numpy as np
import pytest

from oracle.binding import example_tokamak

pytestmark = pytest.mark.gpu

# both contour classes in one chunk (Re omega of both signs: two root entries, two record buffers), several damped
# omegas (deep levels that are one entry wide), the rest near the unstable root
OMEGAS = np.array([-0.8 + 0.25j, 0.5 + 0.1j, -0.6 - 0.21j, -1.656 + 2.49j, 0.153 - 0.316j, -0.7 + 0.3j, -0.9 - 0.8j,
                   -0.5 + 0.2j, 0.3 - 1.1j, -0.65 + 0.27j, -1.0 + 0.05j, -0.4 - 1.5j, 0.7 + 0.4j, -1.2 + 0.35j,
                   -0.75 - 0.5j, 0.2 + 0.02j, -0.85 + 0.15j, -0.55 - 1.2j, 1.1 - 0.3j, -0.95 + 0.4j])

# how the rounds and the chunks fall (the options are those of test_gpu_parity.py's cached-dense cases)
MODES = {
    "planned": dict(node_cache_gb=8.0),
    "all-mfma": dict(node_cache_gb=8.0, dense_min_tasks=0, dense_min_cols=1),
    "all-vector": dict(node_cache_gb=8.0, dense_min_cols=17),  # (up to 16 columns per vector round: no look-ahead beyond two)
    "narrow-chunks": dict(node_cache_gb=8.0, dense_min_tasks=100000000),
    "small-cache": dict(node_cache_gb=0.002, cache_min_depth=1),  # entries outside the cache in mid-level: located, never copied
    "wide": dict(node_cache_gb=8.0, dense_wide=1),  # the 128-entry build (it has no stage: the option must not matter)
}


def _fill(emme, d, stage, options):
    with emme.Context(emme.params_from_dict(d), dense_stage=stage, **options) as ctx:
        M, iv = ctx.assemble(OMEGAS, want_intervals=True)
        out = {"M": M, "iv": iv, "symbol": ctx.fill_kernel_symbol(), "deferred": ctx.last_deferred(),
               "rc": ctx.assemble_rc(OMEGAS)}
        out["M1"], out["iv1"] = ctx.assemble(OMEGAS[11:12], want_intervals=True)  # a chunk of one (damped) omega
    return out


@pytest.mark.parametrize("npoints", [24, 40])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_assembly_is_the_same_bytes_with_and_without_the_stage(emme, npoints, mode):
    d = example_tokamak(npoints=npoints)
    direct, staged = (_fill(emme, d, s, MODES[mode]) for s in (0, 1))
    if mode != "small-cache":  # (the dense fill on both sides, and the option reaches the launcher)
        assert direct["symbol"] == "k_assemble_dense<-1, 15, 1>" and staged["symbol"] == "k_assemble_dense<1, 15, 1>"
    for k in ("M", "M1"):
        assert np.array_equal(direct[k].view(np.float64), staged[k].view(np.float64), equal_nan=True), (mode, npoints, k)
        assert direct[k].tobytes() == staged[k].tobytes(), (mode, npoints, k)
    assert np.array_equal(direct["iv"], staged["iv"]) and np.array_equal(direct["iv1"], staged["iv1"])
    assert direct["rc"] == staged["rc"] and direct["deferred"] == staged["deferred"]
    assert direct["iv"].min() > 0


def test_root_search_is_the_same_bytes_with_and_without_the_stage(emme):
    d = example_tokamak(npoints=24)
    re, im = np.linspace(-1.2, -0.4, 4), np.linspace(0.05, 0.40, 4)
    guesses = (re[None, :] + 1j * im[:, None]).reshape(-1)  # 16 guesses of the bench lattice's window
    res = []
    for stage in (0, 1):
        with emme.Context(emme.params_from_dict(d), dense_stage=stage, node_cache_gb=8.0) as ctx:
            res.append(ctx.solve_roots(guesses, want_iterates=True))
            assert ctx.fill_kernel_symbol().startswith("k_assemble_dense<")
    for a, b in zip(*res):
        assert a.tobytes() == b.tobytes()
    assert (res[0][2] == 0).any()  # (some chain converged: the search did run)
