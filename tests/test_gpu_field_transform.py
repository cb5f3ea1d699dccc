"""Transform 1 of the mode-filter solve (include/pic1dp_hip.h set_field_transform: the FFT, kernels_fft.hip) on the GPU:
against the definition evaluated in extended precision with exactly reduced angles, against transform 0, independent of
npe, in runs through every path, composed with the finite-difference solver, its errors, and the Fortran host's option."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from util import relerr

pytestmark = pytest.mark.gpu


def definition(rho, modes, lx):
    """kept modes and E of the mode-filter solve in np.longdouble: bin b = m mod nx, R + i I = sum rho e^{-2 pi i b ix/nx}
    with the angle (b ix) mod nx reduced in integers; mode_re = I / nx * grad_inv, mode_im = -R / nx * grad_inv,
    E = 2 sum_m (mode_re cos - mode_im sin)"""
    nx = len(rho)
    L = np.longdouble
    q = np.arange(nx)
    th = L(2) * L(np.pi) * q.astype(L) / L(nx)
    cos, sin = np.cos(th), np.sin(th)
    # exact values where the turn is a multiple of a quarter (np.pi is a double: its error would show there)
    cos[(4 * q) % nx == 0] = np.array([1, 0, -1, 0], dtype=L)[(4 * q[(4 * q) % nx == 0]) // nx]
    sin[(4 * q) % nx == 0] = np.array([0, 1, 0, -1], dtype=L)[(4 * q[(4 * q) % nx == 0]) // nx]
    rho_l = np.asarray(rho, dtype=L)
    ix = np.arange(nx, dtype=np.int64)
    modes = np.asarray(modes, dtype=np.int64)
    re, im = np.empty(len(modes), dtype=L), np.empty(len(modes), dtype=L)
    E = np.zeros(nx, dtype=L)
    for a in range(0, len(modes), 128):  # chunks of modes: [128][nx] index tables
        ms = modes[a:a + 128]
        idx = (np.outer(ms % nx, ix)) % nx
        R = (rho_l[None, :] * cos[idx]).sum(axis=1)
        I = -(rho_l[None, :] * sin[idx]).sum(axis=1)
        ginv = L(1) / (L(2) * L(np.pi) / L(lx) * ms.astype(L))
        re[a:a + 128] = I / L(nx) * ginv
        im[a:a + 128] = -R / L(nx) * ginv
        E += L(2) * (re[a:a + 128, None] * cos[idx] - im[a:a + 128, None] * sin[idx]).sum(axis=0)
    return re.astype(np.float64), im.astype(np.float64), E.astype(np.float64)


def mode_lists(nx, seed):
    rng = np.random.default_rng(seed)
    rand = list(rng.integers(1, 4 * nx + 1, size=min(24, 2 * nx)))
    rand += [rand[0], rand[1], max(1, nx // 2), nx, nx + 1, 3 * nx - 1, max(1, nx // 2)]  # duplicates, the aliased bins
    return {"one": [1], "half": list(range(1, nx // 2 + 1)) or [1], "mixed": [int(m) for m in rand]}


def solve(amd, nx, modes, rho, transform, npe=0, field_solver=0):
    eng = amd.Pic1dp(amd.make_input(nparticle_max=16, nx=nx, nmode=len(modes), modes=modes), npe=npe, device=0)
    eng.set_field_solver(field_solver)
    eng.set_field_transform(transform)
    eng.set_chargeden(rho)
    eng.field_solve_electric()
    f = eng.get_field()
    out = (f["mode_re"], f["mode_im"], f["electric"])
    eng.close()
    return out


GRIDS = [2, 3, 64, 100, 192, 1000, 1024, 4096, 8192]


@pytest.mark.parametrize("nx", GRIDS)
def test_fft_against_the_extended_precision_definition(amd, nx):
    lx = amd.make_input().lx
    rng = np.random.default_rng(nx)
    rho = rng.standard_normal(nx) + 0.3
    for name, modes in mode_lists(nx, nx).items():
        re, im, E = solve(amd, nx, modes, rho, 1)
        wre, wim, wE = definition(rho, modes, lx)
        err_m = relerr(np.r_[re, im], np.r_[wre, wim])
        err_e = relerr(E, wE)
        print("nx %5d modes %-5s (%4d): relerr modes %.2e  E %.2e" % (nx, name, len(modes), err_m, err_e))
        assert err_m <= 1e-13, (name, err_m)
        assert err_e <= 1e-13, (name, err_e)


def gaps(a, b):
    """transform 1's result a against transform 0's b: the kept modes relative to their max, E relative to the larger of
    its max and 2 max |mode| (E may vanish: one kept mode at bin nx / 2 and transform 0's sin(pi ix) != 0)"""
    err_m = relerr(np.r_[a[0], a[1]], np.r_[b[0], b[1]])
    scale = max(np.max(np.abs(b[2])), 2 * np.max(np.hypot(b[0], b[1])))
    return err_m, float(np.max(np.abs(a[2] - b[2])) / scale)


@pytest.mark.parametrize("nx", GRIDS)
def test_fft_against_transform_0(amd, nx):
    rng = np.random.default_rng(1000 + nx)
    rho = rng.standard_normal(nx) - 0.2
    lists = mode_lists(nx, 7 * nx)
    # transform 0's tables carry the argument error of cos(2 pi / nx * m * ix), growing with m ix: the bound holds for
    # m <= nx on grids up to 1024; beyond (the mixed list reaches 4 nx, and the large grids) only the gap is logged --
    # test 1 holds both transforms' inputs to the definition there
    lists["upto_nx"] = [m for m in lists["mixed"] if m <= nx]
    for name, modes in lists.items():
        a = solve(amd, nx, modes, rho, 1)
        b = solve(amd, nx, modes, rho, 0)
        err_m, err_e = gaps(a, b)
        print("nx %5d modes %-7s (%4d): transform 1 vs 0 relerr modes %.2e E %.2e" % (nx, name, len(modes), err_m, err_e))
        if nx <= 1024 and name != "mixed":
            assert max(err_m, err_e) <= 1e-12, (name, err_m, err_e)


@pytest.mark.parametrize("nx", [64, 1000, 1024, 8192])
def test_fft_is_independent_of_npe(amd, nx):
    rng = np.random.default_rng(2000 + nx)
    rho = rng.standard_normal(nx)
    for modes in mode_lists(nx, nx).values():
        a = solve(amd, nx, modes, rho, 1, npe=1)
        b = solve(amd, nx, modes, rho, 1, npe=8)
        for x, y in zip(a, b):
            assert np.array_equal(x, y)


def run(amd, nx, nmode, transform, api="step", steps=200, exact=False, switch=False):
    modes = list(range(1, nmode + 1))
    eng = amd.Pic1dp(amd.make_input(nparticle_max=2_000_000, nx=nx, nmode=nmode, modes=modes), device=0)
    eng.particle_load()
    if exact:
        eng.set_charge_sum(1)
    eng.set_field_transform(transform)
    eng.interaction_collect_charge()
    eng.field_solve_electric()
    if api == "step":
        eng.step(steps)
    elif api == "substep":
        for _ in range(steps):
            eng.substep(1)
            eng.substep(2)
    else:
        for _ in range(steps):
            for irk in (1, 2):
                eng.interaction_push_particle(irk)
                eng.interaction_collect_charge()
                if switch:  # a transform switch between collect_charge and solve_field: the solve is transform 1's
                    eng.set_field_transform(0)
                    eng.set_field_transform(1)
                eng.field_solve_electric()
    f = eng.get_field()
    out = dict(E=f["electric"], re=f["mode_re"], im=f["mode_im"], hist=eng.energy_history() if api != "calls" else np.zeros(1))
    eng.close()
    return out


@pytest.mark.parametrize("nx,nmode", [(1024, 512), (192, 1)])
def test_runs_match_transform_0(amd, nx, nmode):
    a = run(amd, nx, nmode, 0)
    b = run(amd, nx, nmode, 1)
    assert len(a["hist"]) == len(b["hist"]) == 200
    err = np.max(np.abs(b["hist"] / a["hist"] - 1.0))
    print("nx %d nmode %d: energy history relerr %.2e" % (nx, nmode, err))
    assert err < 1e-9


CODE = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import numpy as np, pic1dp_amd as amd; "
        "import test_gpu_field_transform as T; r = T.run(amd, 1024, 512, 1, api='calls', steps=20, exact=True, switch=True); "
        "np.savez(%r, **r)")


def test_exact_charge_runs_are_bit_identical_through_every_path(amd, tmp_path):
    base = run(amd, 1024, 512, 1, api="step", steps=20, exact=True)
    for api in ("substep", "calls"):
        assert np.array_equal(run(amd, 1024, 512, 1, api=api, steps=20, exact=True)["E"], base["E"]), api
    lazy = run(amd, 1024, 512, 1, api="calls", steps=20, exact=True, switch=True)
    assert np.array_equal(lazy["E"], base["E"])
    out = str(tmp_path / "eager.npz")
    env = dict(os.environ, PIC1DP_LAZY_CALLS="0")
    subprocess.run([sys.executable, "-c", CODE % (ROOT, os.path.join(ROOT, "tests"), out)], env=env, check=True, timeout=300)
    eager = dict(np.load(out))
    assert np.array_equal(eager["E"], lazy["E"])
    assert np.array_equal(eager["re"], lazy["re"]) and np.array_equal(eager["im"], lazy["im"])


@pytest.mark.parametrize("nx", [64, 1000, 1024])
def test_composes_with_the_finite_difference_solver(amd, nx):
    rng = np.random.default_rng(3000 + nx)
    rho = rng.standard_normal(nx)
    modes = [m for m in mode_lists(nx, nx)["mixed"] if m <= nx]  # (test 2's regime of transform 0's tables)
    a = solve(amd, nx, modes, rho, 0, field_solver=1)
    b = solve(amd, nx, modes, rho, 1, field_solver=1)
    assert np.array_equal(a[2], b[2])  # E: the finite differences, from the same chargeden
    assert relerr(np.r_[b[0], b[1]], np.r_[a[0], a[1]]) <= 1e-12


def test_errors_and_an_unchanged_default(amd):
    eng = amd.Pic1dp(amd.make_input(nparticle_max=16, nx=64), device=0)
    with pytest.raises(amd.Pic1dpError) as e:
        eng.set_field_transform(2)
    assert e.value.code == 1
    odd = amd.Pic1dp(amd.make_input(nparticle_max=16, nx=97), device=0)
    with pytest.raises(amd.Pic1dpError) as e:
        odd.set_field_transform(1)
    assert e.value.code == 1
    rho = np.random.default_rng(5).standard_normal(64)
    never = amd.Pic1dp(amd.make_input(nparticle_max=16, nx=64), device=0)
    for c in (eng, never):
        c.set_chargeden(rho)
    eng.set_field_transform(1)
    eng.set_field_transform(0)
    for c in (eng, never):
        c.field_solve_electric()
    a, b = eng.get_field(), never.get_field()
    for k in ("electric", "mode_re", "mode_im"):
        assert np.array_equal(a[k], b[k])


def test_fortran_host_option(amd, tmp_path):
    exe = os.path.join(ROOT, "pic1dp_amd", "fortran", "pic1dp_host")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.dirname(exe)], capture_output=True, text=True)
    assert os.path.exists(exe), "the Fortran host does not build"
    from pic1dp_amd import output
    env = dict(os.environ, PIC1DP_NPARTICLE="80000", PIC1DP_NX="64", PIC1DP_TIME_MAX="1.0")
    outs = {}
    for tr in ("", "fft"):
        wd = tmp_path / ("t" + tr)
        wd.mkdir()
        r = subprocess.run([exe], cwd=str(wd), env=dict(env, PIC1DP_FIELD_TRANSFORM=tr), capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        outs[tr] = output.OutputData(str(wd / "pic1dp.out"))
    a, b = outs[""], outs["fft"]
    assert a.ntime == b.ntime == 3
    assert np.max(np.abs(b.scalars[:, 1] / a.scalars[:, 1] - 1.0)) < 1e-10
