"""The HIP library against what the reference's own modules computed, with no oracle in between:
tests/golden/ref_hotpath_<case>.npz (written by tests/golden/gen_ref_hotpath.py from the reference's load, deposit, push,
field solve and marker optimisation sources, compiled behind a serial PETSc stand-in; 4 096 markers per case).

Bars: load bit-exact; x and v bit-exact after both pushes, the backup arrays after the first (the engine keeps none
after the second); w bit-exact without exp, else by the
bounds of test_gpu_parity (assert_w_close / assert_w_close_one_exp); chargeden within CHARGE_RTOL, and bit-exact under
set_charge_sum(1) against the exact sum of the reference's per-marker terms; the field solve bit-exact on the
reference's charge density; optimisation events bit-exact.  Through the eager call sites, the lazy call sites and
step().  Reads tests/golden/ only."""
import json
import os

import numpy as np
import pytest

import exact_charge as X
import ref_hotpath as H
from test_gpu_parity import CHARGE_RTOL, assert_w_close, assert_w_close_one_exp, one_exp_active, w_cancellation
from util import relerr

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle", "ref_cases.json")) as _f:
    _CASE_FILE = json.load(_f)
CASES = list(_CASE_FILE["cases"])
EPS = np.finfo(np.float64).eps


def case_kwargs(case):
    """the keywords of the case's 4 096-marker variant (oracle.ref_case_kwargs, restated: the product's tests do not
    need the oracle package for this).  The engine builds iptclshape 4 only: the reference's shape-array variant
    (shape3) is the same arithmetic and its record must be met by the same kernels."""
    kw = dict(_CASE_FILE["base"])
    kw.update(_CASE_FILE["cases"][case])
    kw["nparticle_max"] = kw.pop("fixture_nparticle_max", _CASE_FILE["fixture_nparticle_max"])
    frac = kw.pop("species_nparticle_init_frac", None)
    if frac is not None:
        kw["species_nparticle_init"] = [int(kw["nparticle_max"] * frac)] * kw.get("nspecies", 1)
    kw["iptclshape"] = 4
    return kw


def fixture(case):
    with np.load(H.fixture_path(case)) as f:
        return {k: f[k] for k in f.files}


def check_w(probe, inp, isp, v_at, w_gpu, w_ref, wb_ref):
    """w of species isp after a push from velocities v_at: bit-exact without exp, else the bounds of test_gpu_parity"""
    if H.exp_free(inp):
        H.same_bits(w_gpu, w_ref, "w species %d" % isp)
    elif one_exp_active(probe, inp):
        assert isp == 0
        assert_w_close_one_exp(inp, v_at, w_gpu, w_ref, wb_ref)
    else:
        assert isp == 0
        assert_w_close(w_gpu, w_ref, wb_ref, False, w_cancellation(inp, v_at))


def check_pushed(probe, eng, rec, tag, v_tag, ns):
    for isp in range(ns):
        n = int(rec["np"][isp])
        g = eng.particles_download(isp)
        H.same_bits(g["x"][:n], rec["%s_x%d" % (tag, isp)], "%s x species %d" % (tag, isp))
        H.same_bits(g["v"][:n], rec["%s_v%d" % (tag, isp)], "%s v species %d" % (tag, isp))
        check_w(probe, eng.inp, isp, rec["%s_v%d" % (v_tag, isp)][:n], g["w"][:n], rec["%s_w%d" % (tag, isp)],
                rec["load_w%d" % isp][:n])
        if tag != "p1":
            continue
        # the backup: the engine keeps one between the two pushes only (after the second its slab holds the half-step
        # state; the reference's is not read again before the next first push rewrites it)
        b = eng.particles_download_bak(isp)
        H.same_bits(b["xb"], rec["load_x%d" % isp][:n], "%s xb species %d" % (tag, isp))
        H.same_bits(b["vb"], rec["load_v%d" % isp][:n], "%s vb species %d" % (tag, isp))
        if eng.inp.deltaf == 1:
            H.same_bits(b["wb"], rec["load_w%d" % isp][:n], "%s wb species %d" % (tag, isp))


def check_load(eng, rec, ns):
    for isp in range(ns):
        nalloc, npv = eng.local_sizes(isp)
        assert npv == rec["np"][isp] and nalloc == rec["load_x%d" % isp].size
        g = eng.particles_download(isp)
        for k in "xvpw":
            H.same_bits(g[k][:npv], rec["load_%s%d" % (k, isp)][:npv], "loaded %s species %d" % (k, isp))


@pytest.mark.parametrize("sites", ["eager", "lazy"])
@pytest.mark.parametrize("case", CASES)
def test_call_sites_against_recorded_reference(amd, probe, monkeypatch, case, sites):
    """load, deposit, push 1, deposit, push 2, [event,] deposit, field solve: the reference's call sites one by one,
    run eagerly (PIC1DP_LAZY_CALLS=0) and lazily (the default)"""
    monkeypatch.setenv("PIC1DP_LAZY_CALLS", "1" if sites == "lazy" else "0")
    rec = fixture(case)
    inp = amd.make_input(**case_kwargs(case))
    ns, events = inp.nspecies, H.has_events(inp)
    eng = amd.Pic1dp(inp)
    eng.particle_load()
    check_load(eng, rec, ns)
    if events:
        eng.set_time(*H.EVENT_TIME)
    eng.interaction_collect_charge()
    err = relerr(eng.get_field()["chargeden"], rec["dep0_rho"])
    print("chargeden of the loaded markers: %.3g" % err)
    assert err < CHARGE_RTOL
    for isp in range(ns):
        npv = int(rec["np"][isp])
        H.same_bits(eng.particles_download(isp)["x"][:npv], rec["load_x%d" % isp][:npv], "x after the first deposit")
    for irk in (1, 2):
        eng.set_electric(rec["E%d" % irk])
        eng.interaction_push_particle(irk)
        check_pushed(probe, eng, rec, "p%d" % irk, "load" if irk == 1 else "p1", ns)
        if irk == 1:
            assert not eng.particle_optimize(1)
            eng.interaction_collect_charge()
            for isp in range(ns):
                npv = int(rec["np"][isp])
                H.same_bits(eng.particles_download(isp)["x"][:npv], rec["dep1_x%d" % isp], "wrapped x after push 1")
            err = relerr(eng.get_field()["chargeden"], rec["half_rho"])
            print("chargeden after push 1: %.3g" % err)
            assert err < CHARGE_RTOL
    if events:
        # no exp in the event cases' weight equation: the engine stands at the event with the reference's weights
        assert eng.particle_optimize(2)
        for isp in range(ns):
            _, npv = eng.local_sizes(isp)
            assert npv == rec["ev_np"][isp]
            g = eng.particles_download(isp)
            for k in "xvpw":
                H.same_bits(g[k][:npv], rec["ev_%s%d" % (k, isp)], "%s after the event, species %d" % (k, isp))
        assert not eng.particle_optimize(2)
    eng.interaction_collect_charge()
    for isp in range(ns):
        _, npv = eng.local_sizes(isp)
        H.same_bits(eng.particles_download(isp)["x"][:npv], rec["dep2_x%d" % isp], "wrapped x after push 2")
    err = relerr(eng.get_field()["chargeden"], rec["dep2_rho"])
    print("chargeden after push 2: %.3g" % err)
    # the weights behind it carry the device exp where the distribution has one: the w bound, relative to the
    # update, is far below CHARGE_RTOL of the density (w itself is 1e-5 of p)
    assert err < CHARGE_RTOL
    # field solve on the reference's own charge density
    eng.set_chargeden(rec["dep2_rho"])
    eng.field_solve_electric()
    f = eng.get_field()
    H.same_bits(f["mode_re"], rec["fs_re"], "mode_re")
    H.same_bits(f["mode_im"], rec["fs_im"], "mode_im")
    H.same_bits(f["electric"], rec["fs_E"], "E")
    eng.set_chargeden(rec["half_rho"])
    eng.field_solve_electric()
    H.same_bits(eng.get_field()["electric"], rec["half_E"], "E of the half step")


@pytest.mark.parametrize("case", [c for c in CASES if not any(k in _CASE_FILE["cases"][c] for k in ("nmerge", "nremove", "nsplit"))])
def test_deposits_of_the_reference_markers(amd, case):
    """the reference's own pushed and far-out markers uploaded: wrapped x bit-exact, chargeden within CHARGE_RTOL of the
    reference's sequential sum, and under set_charge_sum(1) bit-exact against the exact sum of the reference's own
    per-marker terms (the event cases deposit through the call sites: their count changes before this stage)"""
    rec = fixture(case)
    inp = amd.make_input(**case_kwargs(case))
    ns = inp.nspecies
    assert not H.has_events(inp)
    for tag, x_of, rho in (("pushed", lambda i: rec["p2_x%d" % i], "dep2_rho"),
                           ("far", lambda i: H.far_positions(rec["dep2_x%d" % i], inp.lx), "far_rho")):
        for kind in (0, 1):
            eng = amd.Pic1dp(inp)
            xs, qs = [], []
            for isp in range(ns):
                n, nalloc = int(rec["np"][isp]), rec["load_x%d" % isp].size
                pad = lambda a: np.concatenate([a, np.zeros(nalloc - a.size)])
                x, w, p = x_of(isp), rec["p2_w%d" % isp], rec["load_p%d" % isp][:n]
                H.assert_defined_in_reference(x, inp.lx)
                eng.particles_upload(pad(x), pad(rec["p2_v%d" % isp]), pad(p), pad(w), ispecies=isp, np_valid=n)
                xs.append(x)
                qs.append(w if inp.deltaf == 1 else p)
            eng.set_charge_sum(kind)
            eng.interaction_collect_charge()
            cd = eng.get_field()["chargeden"]
            if kind == 0:
                err = relerr(cd, rec[rho])
                print("%s markers, chargeden: %.3g" % (tag, err))
                assert err < CHARGE_RTOL
                for isp in range(ns):
                    n = int(rec["np"][isp])
                    want = rec["dep2_x%d" % isp] if tag == "pushed" else rec["far_x%d" % isp]
                    H.same_bits(eng.particles_download(isp)["x"][:n], want, "wrapped x of the %s markers" % tag)
            else:
                es = [amd.charge_quantum(inp, s) for s in range(ns)]
                want, _, _ = X.exact_chargeden(xs, qs, inp, es)
                H.same_bits(cd, want, "exact chargeden of the %s markers" % tag)
            eng.close()


def field_response_bound(inp, rec, drho):
    """|dE| per |d chargeden| <= drho of the mode-filter solve: each mode amplitude is a mean of +-rho (<= drho) times
    grad_inv, the inverse adds 2 (|re| + |im|) per mode: 4 sum(grad_inv) drho"""
    return 4.0 * float(np.sum(np.abs(rec["grad_inv"]))) * drho


@pytest.mark.parametrize("case", CASES)
def test_step_against_recorded_reference(amd, probe, case):
    """step(1) from the loaded state with the reference's imposed field: x bit-exact (it depends on the imposed field
    alone; the whole-step kernels keep no backup to compare); v and w see the half-step field, which the engine solves from its own charge sum --
    within CHARGE_RTOL of the reference's (asserted here through the half-step field) -- so v within dt |Z/m| dE of the
    reference, dE the field response bound to CHARGE_RTOL max|chargeden|, plus an ulp; w within its bound plus its update
    scaled by dE over the field at the marker"""
    rec = fixture(case)
    inp = amd.make_input(**case_kwargs(case))
    ns, nx, lx = inp.nspecies, inp.nx, inp.lx
    eng = amd.Pic1dp(inp)
    eng.particle_load()
    check_load(eng, rec, ns)
    eng.interaction_collect_charge()
    eng.field_solve_electric()
    eng.set_electric(rec["E1"])
    eng.step(1)
    dE = field_response_bound(inp, rec, CHARGE_RTOL * float(np.max(np.abs(rec["half_rho"]))))
    got_half = eng.get_field_half()
    print("half-step field: off by %.3g, bound %.3g" % (np.max(np.abs(got_half - rec["half_E"])), dE))
    assert np.max(np.abs(got_half - rec["half_E"])) <= dE
    for isp in range(ns):
        n = int(rec["np"][isp])
        zm = abs(inp.species_charge[isp] / inp.species_mass[isp])
        g = eng.particles_download(isp)
        H.same_bits(g["x"][:n], rec["st_x%d" % isp], "x after one step, species %d" % isp)
        v_ref, w_ref = rec["st_v%d" % isp], rec["st_w%d" % isp]
        if inp.linear == 1:
            H.same_bits(g["v"][:n], v_ref, "v (not pushed in a linear run)")
        else:
            tol = inp.dt * zm * dE + 2 * EPS * np.abs(v_ref)
            err = np.abs(g["v"][:n] - v_ref)
            print("v species %d: off by %.3g, smallest bound %.3g" % (isp, err.max(), tol.min()))
            assert np.all(err <= tol)
        if inp.deltaf == 0:
            H.same_bits(g["w"][:n], w_ref, "w (not evolved in full-f)")
            continue
        # the field at the half-step position, as the push gathers it (src/pic1dp_interaction.F90:250-257)
        s = rec["dep1_x%d" % isp] / lx * nx
        ix = np.floor(s).astype(np.int64)
        wl = 1.0 - (s - ix)
        E_p = rec["half_E"][ix] * wl + rec["half_E"][(ix + 1) % nx] * (1.0 - wl)
        wb = rec["load_w%d" % isp][:n]
        upd = np.abs(w_ref - wb)
        with np.errstate(divide="ignore", invalid="ignore"):
            gain = np.where(E_p != 0.0, upd / np.abs(E_p), 0.0)
        extra = np.where(E_p != 0.0, gain, gain.max()) * dE
        err = np.abs(g["w"][:n] - w_ref)
        if H.exp_free(inp):
            tol = extra + 4 * EPS * upd + EPS * np.abs(w_ref)
            print("w species %d: off by %.3g, smallest bound %.3g" % (isp, err.max(), tol.min()))
            assert np.all(err <= tol)
        else:
            # the parity bounds on what is left once at most `extra` is taken off as the field's part
            diff = g["w"][:n] - w_ref
            rest = diff - np.clip(diff, -extra, extra)
            print("w species %d: off by %.3g, of which not the field's %.3g" % (isp, np.abs(diff).max(), np.abs(rest).max()))
            check_w(probe, inp, isp, rec["p1_v%d" % isp], w_ref + rest, w_ref, wb)
