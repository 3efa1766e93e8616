"""CPU: self-checks of the test helper tests/_gp_ref.py, NOT of the library (nothing here calls it): the float64 solves it
restates, and its float32 emulation of the blocked algorithm (full and appended factorisation, both solves, columns completed,
the failed pivot). The emulation is what the Gaussian-process cases were chosen with; tests/test_gpu_gp.py checks the HIP
drivers themselves."""

import numpy as np
import pytest
import torch

import _gp_ref as gref


def test_solves_restated():
    g = torch.Generator().manual_seed(3)
    a = gref.spd(9, 5)
    l = gref.cholesky(a)
    b = torch.randn(4, 9, generator=g, dtype=torch.float64)
    assert torch.allclose(gref.solve_right(l, b) @ l.t(), b, atol=1e-12)
    assert torch.allclose(gref.solve_right(l, b, transposed=True) @ l, b, atol=1e-12)
    assert float(torch.linalg.cond(gref.spd(321, 1).double())) <= 5.1


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 130, 200])
def test_emulated_factorisation_full_and_appended(n):
    a = gref.spd(n, n)
    want = gref.cholesky(a).numpy()
    marker = np.triu(np.full((n, n), 7.0, dtype=np.float32), 1)
    full = np.tril(a.numpy()) + marker
    info = [0]
    gref.emu_potrf(full, 0, info)
    assert info == [0] and np.array_equal(np.triu(full, 1), marker)
    assert np.abs(np.tril(full) - want).max() <= 2e-6 * np.abs(want).max()
    for done in (1, 60, 63, 64, 65, 128, 129):
        if done >= n:
            continue
        part = np.tril(a.numpy()) + marker
        part[:done, :done] = np.tril(full[:done, :done]) + marker[:done, :done]
        gref.emu_potrf(part, done, info)
        assert info == [0] and np.array_equal(np.triu(part, 1), marker)
        assert np.abs(part - full).max() <= 1e-6 * np.abs(want).max(), (n, done)


@pytest.mark.parametrize("n", [1, 2, 65, 130, 200])
def test_emulated_solves(n):
    rng = np.random.default_rng(n)
    l = np.tril(gref.cholesky(gref.spd(n, n)).numpy()).astype(np.float32)
    for rows in (1, 3):
        b = rng.standard_normal((rows, n)).astype(np.float32)
        x = b.copy()
        gref.emu_trsm_right(l, x)
        want = gref.solve_right(torch.tensor(l), torch.tensor(b)).numpy()
        assert np.abs(x - want).max() <= 1e-5 * np.abs(want).max()
        y = b.copy()
        gref.emu_trsm_right(l, y, transposed=True)
        want = gref.solve_right(torch.tensor(l), torch.tensor(b), transposed=True).numpy()
        assert np.abs(y - want).max() <= 1e-5 * np.abs(want).max()
        for done in (1, 63, 64, 65, 129):
            if done >= n:
                continue
            z = b.copy()
            z[:, :done] = x[:, :done]
            gref.emu_trsm_right(l, z, col_done=done)
            assert np.abs(z - x).max() <= 2e-6 * np.abs(x).max(), (n, rows, done)


def test_emulated_failed_pivot():
    a = gref.spd(100, 1).numpy().copy()
    a[70, 70] = -5.0
    info = [0]
    gref.emu_potrf(a, 0, info)
    assert info == [71]
