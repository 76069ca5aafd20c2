"""The premises of test_gpu_linalg_routes.py, checked on the CPU at small orders: the dispatch edge the LDS formula
gives, the shared input families of linalg_cases.py against numpy's SVD and solve, the symmetry structured_pair
promises, and the singular-half constructions -- singular in the half and at the column the GPU test demands."""
import numpy as np
import pytest

import linalg_cases as lc
from fold_reference import folded_trace, structured_pair


def test_the_lds_formula_puts_the_edge_at_525():
    assert lc.blocked_lds_bytes(525) == 9591 * 16 <= lc.LDS_LIMIT < lc.blocked_lds_bytes(526) == 9609 * 16
    assert lc.lds_edge() == 525


def test_expected_routes():
    assert lc.expected_trace_route(525, 1, 384) == lc.ONE_WG
    assert lc.expected_trace_route(525, 2, 384) == lc.GROUPED
    assert lc.expected_trace_route(300, 2, 384) == lc.SPLIT
    assert lc.expected_trace_route(525, 2, -1) == lc.SPLIT
    assert lc.expected_trace_route(525, 8, 384) == lc.SPLIT
    assert lc.expected_trace_route(525, 8, 384, resident=False) == lc.ONE_WG
    assert lc.expected_trace_route(526, 1, 384) == lc.UNBLOCKED
    assert lc.expected_trace_route(526, 8, 384) == lc.CHUNKED
    assert lc.expected_trace_route(526, 16, 384, resident=False) == lc.UNBLOCKED
    assert lc.expected_trace_route(1024, 2, 384) == lc.CHUNKED
    assert lc.expected_trace_route(1025, 8, 384) == lc.UNBLOCKED
    # what trace_solve asks for by default (linstep_plan.hpp): one matrix, many matrices, and the chunked build's two
    assert [lc.lu_workgroups(n, 1, 256) for n in (100, 128, 383, 384, 525, 526, 767, 768, 1024)] == [1, 4, 4, 8, 8, 8, 8, 16, 16]
    assert lc.lu_workgroups(256, 128, 256) == 2 and lc.lu_workgroups(256, 200, 256) == 1
    assert lc.lu_workgroups(526, 200, 256) == 2 and lc.lu_workgroups(526, 200, 256, lu_split=1) == 1
    assert lc.lu_workgroups(300, 3, 256, lu_split=40) == 16
    assert [lc.expected_lu_route(n) for n in (525, 526, 1024, 1025)] == \
        [lc.LU_INPLACE, lc.CHUNKED, lc.CHUNKED, lc.LU_UNBLOCKED]


def test_route_getters_exist_and_refuse_a_null_context(emme):
    import os
    lib = emme.load()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "emme_hip.h")).read()
    for name in ("emme_ctx_linstep_kernel_symbol", "emme_ctx_last_lu_workgroups", "emme_ctx_last_lu_slices",
                 "emme_ctx_compute_units"):
        assert hasattr(lib, name) and name in hdr, name
    assert lib.emme_ctx_linstep_kernel_symbol(None) is None
    assert lib.emme_ctx_last_lu_workgroups(None) == -1 and lib.emme_ctx_last_lu_slices(None) == -1
    assert lib.emme_ctx_compute_units(None) == -1
    for name in ("linstep_kernel_symbol", "last_lu_workgroups", "last_lu_slices", "compute_units"):
        assert callable(getattr(emme.Context, name)), name
    # the symbols the tests compare against are the ones the header documents
    for sym in (lc.ONE_WG, lc.SPLIT, lc.CHUNKED, lc.GROUPED, lc.UNBLOCKED, lc.LU_INPLACE, lc.LU_UNBLOCKED):
        assert '"%s"' % sym in hdr, sym


def test_families_are_built_once_and_read_only():
    A, B, want = lc.shifted_symmetric(12)
    assert lc.shifted_symmetric(12)[0] is A
    with pytest.raises(ValueError):
        A[0, 0, 0] = 0.0
    assert np.array_equal(A, np.transpose(A, (0, 2, 1)))
    assert abs(want[1] - np.trace(np.linalg.inv(A[1]) @ B[1])) <= 1e-12 * abs(want[1])


@pytest.mark.parametrize("n", [5, 33])
def test_null_family_vector_is_numpys(n):
    M, want = lc.null_family(n)
    for b in range(M.shape[0]):
        sv_vec = np.linalg.svd(M[b])[2][-1].conj()
        assert 1.0 - lc.overlap(sv_vec, want[b]) <= 1e-10, (n, b)
    sv = np.linalg.svd(M[0], compute_uv=False)
    assert abs(sv[-1] - 1e-4) <= 1e-12 and 0.3 <= sv[-2] <= sv[0] <= 3.0


def test_constructed_condition_number():
    M, Mp, v, kappa = lc.constructed(24)
    assert np.allclose(kappa, 1e3, rtol=1e-9)
    assert np.allclose(np.linalg.norm(v, axis=1), 1.0)


@pytest.mark.parametrize("n", [6, 33])
def test_pdm_family(n):
    """Every member has its base matrix's singular values, its null vector is numpy's SVD vector, neighbours differ,
    and the solves through the base matrix are numpy's solves of the member."""
    nb = 5
    F = lc.pdm_family(n, nb)
    rng = np.random.default_rng(n)
    V = rng.normal(size=(n, 3)) + 1j * rng.normal(size=(n, 3))
    z, w = rng.normal(size=nb) + 1j * rng.normal(size=nb), rng.normal(size=nb) + 1j * rng.normal(size=nb)
    direct_all = np.array([np.linalg.solve(F.M[b], V) for b in range(nb)])
    for items in (None, [1, 2, 4]):
        R0, R1 = F.moments(V, z, w, items)
        sel = slice(None) if items is None else items
        D0, D1 = lc.moments_of(direct_all[sel], z[sel], w[sel])
        assert np.linalg.norm(R0 - D0) <= 1e-9 * np.linalg.norm(D0) and np.linalg.norm(R1 - D1) <= 1e-9 * np.linalg.norm(D1)
    for b in range(nb):
        base = F.base[b % 2]
        assert np.abs(F.M[b] - F.phase[b][:, None] * base[F.perm[b]]).max() <= 4 * lc.EPS * np.abs(base).max()
        assert np.allclose(np.abs(F.phase[b]), 1.0, rtol=0, atol=1e-15)
        assert sorted(F.perm[b]) == list(range(n))
        sv, sv0 = np.linalg.svd(F.M[b], compute_uv=False), np.linalg.svd(base, compute_uv=False)
        assert np.abs(sv - sv0).max() <= 1e-13 * sv0[0]
        assert abs(sv0[0] / sv0[-1] - F.kappa[b % 2]) <= 1e-6 * F.kappa[b % 2]
        vec = np.linalg.svd(F.M[b])[2][-1].conj()
        assert 1.0 - lc.overlap(vec, F.want[b % 2]) <= 1e-10, (n, b)
        direct = direct_all[b]
        scale = np.linalg.norm(direct)
        assert np.linalg.norm(F.solve(b, V) - direct) <= 1e-9 * scale
        assert np.linalg.norm(F.solve(b, V[:, 0]) - direct[:, 0]) <= 1e-9 * scale
    assert lc.overlap(F.want[0], F.want[1]) < 0.9  # an item's neighbour has another null vector


@pytest.mark.parametrize("n", [16, 30])
def test_structured_pair_symmetry(n):
    """Symmetric, and centrosymmetric apart from the last row and column: C = M - (u e^T + e u^T) with the edge u the
    fold reads is centrosymmetric, and so are the halves' sources."""
    rng = np.random.default_rng(n)
    for X in structured_pair(rng, n):
        assert np.array_equal(X, X.T)
        _, _, u = lc.fold_halves(X)
        E = np.zeros_like(X)
        E[:, n - 1] += u
        E[n - 1, :] += u
        C = X - E
        assert np.abs(C - C[::-1, ::-1]).max() <= 1e-13 * np.abs(X).max()
    M, Mo, dw, ref = lc.fold_inputs(n, 2)
    for b in range(2):
        got = folded_trace(M[b], Mo[b], dw[b])
        assert abs(got - ref[b]) <= 1e-10 * abs(ref[b])


@pytest.mark.parametrize("odd", [False, True])
@pytest.mark.parametrize("n,k", [(16, 1), (16, 5), (16, 7), (130, 1), (130, 16), (130, 40), (130, 64)])
def test_singular_half_constructions(n, k, odd):
    """The chosen half has an exactly zero row and column k, its partial-pivot LU stops at column k + 1 and the other
    half's runs through; the matrix stays symmetric."""
    M = lc.fold_inputs(n, 3)[0][1]
    X = lc.with_singular_half(M, k, odd)
    assert np.array_equal(X, X.T)
    Sp, Sm, _ = lc.fold_halves(X)
    hit, other = (Sm, Sp) if odd else (Sp, Sm)
    assert not hit[:, k].any() and not hit[k, :].any()
    assert np.count_nonzero(np.abs(hit).sum(axis=0) == 0.0) == 1
    assert lc.lu_stop_column(hit) == k + 1
    assert lc.lu_stop_column(other) == 0


@pytest.mark.parametrize("n", [16, 130])
def test_exactly_singular_k(n):
    """det K = 0 bit for bit with both halves regular; the matrix itself is singular at its last column."""
    M, Mo = lc.singular_k_matrix(n)
    Sp, Sm, u = lc.fold_halves(M)
    assert lc.lu_stop_column(Sp) == 0 and lc.lu_stop_column(Sm) == 0
    assert u[n - 1] == -1.0 and not u[:n - 1].any()
    K = lc.fold_k_matrix(M)
    assert np.array_equal(K, np.full((2, 2), 0.5 + 0.0j))
    assert K[0, 0] * K[1, 1] - K[0, 1] * K[1, 0] == 0.0
    assert lc.lu_stop_column(M) == n
    assert np.array_equal(Mo, Mo.T)


def test_lu_stop_column_is_the_first_zero_pivot():
    rng = np.random.default_rng(3)
    A = rng.normal(size=(9, 9)) + 1j * rng.normal(size=(9, 9))
    assert lc.lu_stop_column(A) == 0
    A[:, 4] = 0.0
    assert lc.lu_stop_column(A) == 5
