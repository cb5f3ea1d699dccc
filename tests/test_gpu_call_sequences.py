"""Differential test of the on-demand marker products and the restart INSIDE the state machine of the lazy call sites,
the one-pass prediction and the pair solve: the random call sequences of tests/call_sequences.py -- the
reference's push(1), collect_charge, solve_field, push(2), collect_charge, solve_field with intruders at every boundary
B0 ... B5 and between charge_local and charge_reduced (P) -- on three engines, every call followed by a deep check_state:

    a   the default engine: lazy call sites and the mode's prediction (tiles, six sums; none with the exact charge sum)
    b   every call eager, two marker passes per step (PIC1DP_LAZY_CALLS=0, PIC1DP_PREDICT=0)
    c   configured as a, running the same sequence WITHOUT the read-only intruders

At every read-only intruder (moments, moments_local_exact, power, power_local_exact, select, select_count, gather,
state_digest, output_all, checkpoint): the same return code on a and b (at P a product may be refused with
PIC1DP_ERR_STATE, on both or on neither); the result against an independent reference computed from b's own
particles_download -- and, where the markers of a and b agree only to 1e-10 (tiles, sums), a's result against the reference
from a's own download taken right after the call, the float products of a and b within the sum of their two bounds plus
1e-10 of the plane's maximum --; the state digest before and after the call equal on the same engine.  With the exact
charge sum and the exact diagnostics sum a's result has to pass the very check against b's reference without a download on
a, and the integer products, the selections, the gathered markers, the digest and the whole output_all record are bit for
bit those of b.  The references that sum with math.fsum or in Python integers (moments, power and their exact kinds) are
evaluated at most call_sequences.MAX_REFERENCES times per seed; which intrusions get them is chosen by (kind, place) for a
mode's seeds together (call_sequences.referenced), so that every pair is held against its reference in at least one seed --
tests/test_call_sequences_host.py asserts that.  At every other intrusion of those kinds the bounds alone are computed
(numpy) and the engines are held against each other: the float products of a and b within the sum of their bounds (plus
1e-10 where the markers differ), the exact kinds bit for bit, or, where the markers differ, converted to doubles within
one quantum per term plus 1e-10.

The checkpoint: at B0 a write, then a restart from the file on a and on b (the old contexts closed), bit for bit the state
that was written; inside a time step and at P the write is refused with PIC1DP_ERR_STATE, leaves no file, and the context
goes on.  At the looks the older differential has (`download`) and at the end, twice, markers, E, the kept modes, chargeden
by its flag and the energy history of a against b -- 1e-10, or bit for bit with the exact sums; at the end c against a the
same way: a product that disturbed the state in the same way on a and on b shows there.

Every assertion message carries the last ten calls.  A longer campaign: PIC1DP_FUZZ_BASE / PIC1DP_FUZZ_MULT as in
tests/test_gpu_fuzz.py."""
import collections
import math
import os

import numpy as np
import pytest

import call_sequences as CS
import moments_exact as MX
import moments_reference as MR
import power_exact as PX
import power_reference as PR
import select_reference as SR
from test_gpu_fuzz import Checked, _Compare, _kept_coefficients, _two_engines, seeds

pytestmark = pytest.mark.gpu

ERR_STATE = 4
FIELD_KEYS = ("electric", "chargeden", "mode_re", "mode_im")
DIST_KEYS = ("markr_xv", "total_xv", "pertb_xv", "markr_v", "total_v", "pertb_v")


def _cut(g, n):
    return [g[k][:n] for k in "xvpw"]


def _moments_bounds(g, npv, inp, which):
    """{"total" / "pertb": dict(abs, count)}: what MR.bound needs, without the exact sums"""
    x, v, p, w = _cut(g, npv)
    out = {}
    for bit, name, q in ((1, "total", p), (2, "pertb", w)):
        if which & bit:
            cell, ts = MR.terms(x, v, q, inp)
            out[name] = dict(abs=np.stack([np.bincount(cell, weights=np.abs(t), minlength=inp.nx) for t in ts]),
                             count=np.bincount(cell, minlength=inp.nx))
    return out


def _power_bounds(g, npv, E, inp, which):
    """{"total" / "pertb": dict(abs, count, rest)}: what PR.bound, bound_v and bound_rest need, without the exact sums"""
    x, v, p, w = _cut(g, npv)
    nxo, nvo = inp.nx_opd, inp.nv_opd
    out = {}
    for bit, name, q in ((1, "total", p), (2, "pertb", w)):
        if which & bit:
            cell, t, rt = PR.terms(x, v, q, E, inp)
            out[name] = dict(abs=np.bincount(cell, weights=np.abs(t), minlength=nxo * nvo).reshape(nvo, nxo),
                             count=np.bincount(cell, minlength=nxo * nvo).reshape(nvo, nxo),
                             rest=dict(abs=float(np.sum(np.abs(rt))), count=int(rt.size)))
    return out


def _power_v_bound(ref_set, nwg):
    """the v-profile against the exact row sums (tests/test_gpu_power.py within): bound_v, and the rounding of the
    reference's own bins that the exact row sum does not carry.  `within` takes nx_opd 2^-53 sum |exact bins| for the
    latter; here it is nx_opd 2^-53 sum |terms|, which is no smaller (|exact| <= abs bin by bin, a difference at the level
    of 1e-16 of the row) and needs no exact sums, so the same bound serves where only the bounds are computed"""
    return PR.bound_v(ref_set, nwg) + ref_set["abs"].shape[1] * PR.U * ref_set["abs"].sum(axis=1)


class _Run:
    def __init__(self, amd, monkeypatch, tmp_path, mode, seed):
        self.amd, self.mp, self.tmp, self.mode = amd, monkeypatch, tmp_path, mode
        self.seq = CS.sequence(seed, mode)
        self.kind, self.exact = CS.KIND[mode], mode == "exact"
        kw, npe = self.seq["kw"], self.seq["npe"]
        self.nsp = self.seq["nspecies"]
        self.a, self.b = _two_engines(amd, monkeypatch, kw, self.kind, npe)
        self.c = self.like_a(lambda: amd.Pic1dp(amd.make_input(**kw), npe=npe))
        self.inp = self.b.inp
        self.log = []
        self.cmp = _Compare(self.a, self.b, self.kind or 1, kw["modes"], self.exact, self.log)
        self.referenced = CS.referenced(seed, mode)[0]    # ordinals of the intrusions held against the fsum / integer references
        self.ordinal, self.full = 0, False
        self.ran = collections.Counter()
        self.nckpt = 0
        for e in (self.a, self.b, self.c):
            e.particle_load_device(1) if self.seq["load"] == "device" else e.particle_load()
            if self.exact:
                e.set_charge_sum(1)
                e.set_diag_sum(1)
            e.interaction_collect_charge()
            e.field_solve_electric()
        assert self.b.predict_kind() == 0
        if self.seq["pair_case"]:
            assert self.a.predict_kind() == 2
        for isp in range(self.nsp):
            assert self.b.local_sizes(isp)[0] == kw["nparticle_max"]     # (what the generator's gather indices assume)
        self.skips, self.skips0 = 0, self.a.kernel_stats(11)[1]

    # -- engines ----------------------------------------------------------------
    def like_a(self, make):
        if self.kind:
            self.mp.setenv("PIC1DP_PRED_KIND", str(self.kind))
        e = Checked(make())
        if self.kind:
            self.mp.delenv("PIC1DP_PRED_KIND")
        return e

    def like_b(self, make):
        self.mp.setenv("PIC1DP_LAZY_CALLS", "0")
        self.mp.setenv("PIC1DP_PREDICT", "0")
        e = Checked(make())
        self.mp.delenv("PIC1DP_LAZY_CALLS")
        self.mp.delenv("PIC1DP_PREDICT")
        return e

    def tail(self):
        return self.log[-10:]

    def call(self, e, f):
        try:
            return 0, f(e)
        except self.amd.Pic1dpError as err:
            e.check_state(True)
            return err.code, None

    def bracket(self, e, f, what):
        """(code, result) of f(e) between two state digests, which have to be equal: the call changes no marker.  (The first
        digest has already put a noted push into memory.)"""
        d0 = e.state_digest()
        code, out = self.call(e, f)
        d1 = e.state_digest()
        assert np.array_equal(d0, d1), (what, "changed the markers", self.tail())
        return code, out

    def down(self, e, isp):
        return e.particles_download(isp), e.local_sizes(isp)[1]

    def sources(self, isp):
        """[(result index, download, valid markers, engine)]: whose markers the reference is computed from, for a's result
        (0) and for b's (1) -- b's download for both with the exact sums (no download on a)"""
        gb, nb = self.down(self.b, isp)
        if self.exact:
            return [(0, gb, nb, self.b), (1, gb, nb, self.b)]
        ga, na = self.down(self.a, isp)
        return [(0, ga, na, self.a), (1, gb, nb, self.b)]

    # -- the looks ----------------------------------------------------------------
    def markers(self, cmp, tag):
        for isp in range(self.nsp):
            ga, gb = cmp.a.particles_download(isp), cmp.b.particles_download(isp)
            for k in "xvw":
                cmp.close(ga[k], gb[k], (tag, isp, k))

    def field_by_both_flags(self, cmp, tag):
        """_Compare.field with chargeden for two engines that may BOTH hold a half step's kept modes only (both lazy): the
        whole vector if both say it is the reference's, the kept modes' coefficients otherwise"""
        fa, fb = cmp.a.get_field(), cmp.b.get_field()
        for k in ("electric", "mode_re", "mode_im"):
            cmp.close(fa[k], fb[k], (tag, k))
        if not (cmp.a.chargeden_kept_mode_only() or cmp.b.chargeden_kept_mode_only()):
            cmp.close(fa["chargeden"], fb["chargeden"], (tag, "chargeden"))
            return
        assert self.kind == 2 and not self.exact, (tag, "kept-mode-only chargeden outside the six sums", self.tail())
        ca, cb = (_kept_coefficients(f["chargeden"], self.seq["kw"]["modes"]) for f in (fa, fb))
        scale = max(np.max(np.abs(cb)), np.max(np.abs(fb["chargeden"])), 1e-300)
        assert np.max(np.abs(ca - cb)) <= 1e-10 * scale, (tag, "kept modes of chargeden", self.tail())

    # -- read-only intruders --------------------------------------------------------
    def read_only(self, kind, args):
        at = args["at"]
        self.log.append("%s@%s" % (kind, at))
        # (call_sequences.referenced: at most MAX_REFERENCES evaluations per seed, every (kind, place) at least once per mode)
        self.full = self.ordinal in self.referenced
        self.ordinal += 1
        if kind == "checkpoint":
            return self.checkpoint(args)
        f = getattr(self, "do_" + kind)(args)
        ca, ra = self.bracket(self.a, f, kind)
        cb, rb = self.bracket(self.b, f, kind)
        assert ca == cb, (kind, "return codes differ", ca, cb, self.tail())
        # include/pic1dp_hip.h, "When the call may come": between charge_local and charge_reduced every product is served as
        # particles_download is, and output_all alone is refused
        want = ERR_STATE if (at == "P" and kind == "output_all") else 0
        assert ca == want, (kind, "return code", ca, "expected", want, self.tail())
        self.ran[(kind, at, "ran" if ca == 0 else "refused")] += 1
        if ca == 0:
            getattr(self, "check_" + kind)(args, ra, rb)

    def do_moments(self, args):
        return lambda e: e.moments(args["isp"], args["which"])

    def check_moments(self, args, ra, rb):
        isp, which = args["isp"], args["which"]
        full = self.full
        src = self.sources(isp)
        sets = []
        for i, g, n, _ in src:
            if i == 1 and self.exact:
                sets.append(sets[0])
                continue
            sets.append(MR.reference(*_cut(g, n), self.inp, which) if full else _moments_bounds(g, n, self.inp, which))
        bounds = [{name: MR.bound(s[name], MR.workgroups(n)) for name in s} for s, (_, _, n, _) in zip(sets, src)]
        for name in sets[0]:
            if full:
                for got, s, b, who in zip((ra, rb), sets, bounds, "ab"):
                    err = np.abs(got[name] - s[name]["exact"])
                    assert np.all(err <= b[name]), ("moments", who, name, float(np.max(err - b[name])), self.tail())
            # always, engine against engine: each within its bound of the exact sum of its own markers' terms; the markers
            # are the same with the exact sums, and agree to 1e-10 otherwise
            tol = bounds[0][name] + bounds[1][name]
            if not self.exact:
                tol = tol + 1e-10 * np.max(np.abs(rb[name]), axis=1, keepdims=True)
            assert np.all(np.abs(ra[name] - rb[name]) <= tol), ("moments a against b", name, self.tail())

    def do_moments_local_exact(self, args):
        return lambda e: e.moments_local_exact(args["isp"], args["which"])

    def check_moments_local_exact(self, args, ra, rb):
        isp, which = args["isp"], args["which"]
        src = self.sources(isp)
        if self.exact:
            assert np.array_equal(ra, rb), ("moments_local_exact a against b", self.tail())
        else:
            # always, engine against engine: the integer sums are exact, so they differ only through the markers, which
            # agree to 1e-10 -- 1e-10 of the plane's maximum, and one quantum 2^e[k] for every term of the bin, since a term
            # that moves by less than a quantum may still round to the next one; the conversion rounds each side once
            da, db = (self.amd.moments_convert(self.inp, r, which, isp) for r in (ra, rb))
            q = np.ldexp(1.0, np.array(MX.quanta(self.inp, isp)))[:, None]
            count = _moments_bounds(src[1][1], src[1][2], self.inp, which)
            for name in db:
                tol = (count[name]["count"][None, :] * q + 1e-10 * np.max(np.abs(db[name]), axis=1, keepdims=True)
                       + 2.0 * MR.U * np.abs(db[name]))
                assert np.all(np.abs(da[name] - db[name]) <= tol), ("moments_local_exact a against b", name, self.tail())
        if not self.full:
            return
        refs = [MX.reference(*_cut(src[0][1], src[0][2]), self.inp, which, isp)]
        refs.append(refs[0] if self.exact else MX.reference(*_cut(src[1][1], src[1][2]), self.inp, which, isp))
        for got, ref, who in zip((ra, rb), refs, "ab"):
            assert got.dtype == np.int64 and np.array_equal(got, ref["limbs"]), ("moments_local_exact", who, self.tail())

    def do_power(self, args):
        return lambda e: e.power(args["isp"], args["which"])

    def check_power(self, args, ra, rb):
        isp, which = args["isp"], args["which"]
        full = self.full
        src = self.sources(isp)
        sets = []
        for i, g, n, e in src:
            if i == 1 and self.exact:
                sets.append(sets[0])
                continue
            E = e.get_field(chargeden=False)["electric"]
            sets.append(PR.reference(*_cut(g, n), E, self.inp, which) if full else _power_bounds(g, n, E, self.inp, which))
        nwg = [PR.workgroups(n) for _, _, n, _ in src]
        for name in sets[0]:
            b_xv = [PR.bound(s[name], w) for s, w in zip(sets, nwg)]
            b_v = [_power_v_bound(s[name], w) for s, w in zip(sets, nwg)]
            b_rest = [PR.bound_rest(s[name], w) for s, w in zip(sets, nwg)]
            if full:
                for j, (got, s, who) in enumerate(zip((ra, rb), sets, "ab")):
                    s = s[name]
                    rows = np.array([math.fsum(row) for row in s["exact"].tolist()])
                    for key, err, b in (("xv", np.abs(got[name]["xv"] - s["exact"]), b_xv[j]),
                                        ("v", np.abs(got[name]["v"] - rows), b_v[j]),
                                        ("rest", np.abs(got[name]["rest"] - s["rest"]["exact"]), b_rest[j])):
                        assert np.all(err <= b), ("power", who, name, key, float(np.max(err - b)), self.tail())
            # always, engine against engine: each within its bounds of the exact sums of its own markers' terms; the markers
            # (and the field) are the same with the exact sums, and agree to 1e-10 otherwise.  (rest is one sum of terms of
            # both signs: its 1e-10 is that of its terms, as for sum v^2 w in tests/test_gpu_fuzz.py -- with the few markers
            # beyond v_max there are, a bar relative to the sum itself would be one relative to a cancellation)
            ga, gb = ra[name], rb[name]
            slack = 0.0 if self.exact else 1e-10
            assert np.all(np.abs(ga["xv"] - gb["xv"]) <= b_xv[0] + b_xv[1] + slack * np.max(np.abs(gb["xv"]))), \
                ("power a against b", name, "xv", self.tail())
            assert np.all(np.abs(ga["v"] - gb["v"]) <= b_v[0] + b_v[1] + slack * np.max(np.abs(gb["v"]))), \
                ("power a against b", name, "v", self.tail())
            assert abs(ga["rest"] - gb["rest"]) <= b_rest[0] + b_rest[1] + slack * sets[1][name]["rest"]["abs"], \
                ("power a against b", name, "rest", self.tail())

    def do_power_local_exact(self, args):
        return lambda e: e.power_local_exact(args["isp"], args["which"])

    def check_power_local_exact(self, args, ra, rb):
        isp, which = args["isp"], args["which"]
        if self.exact:
            assert ra[1] == rb[1] and np.array_equal(ra[0], rb[0]), ("power_local_exact a against b", self.tail())
        else:
            # always, engine against engine, as for moments_local_exact: one quantum for every term of the bin (of the row,
            # of rest) and 1e-10 of the plane's maximum (of the sum of |terms| for rest); the quantum is the larger of the two
            # calls' (max |E| of a and b may lie on either side of a power of two)
            da, db = (self.amd.power_convert(self.inp, r[0], r[1], which) for r in (ra, rb))
            q = math.ldexp(1.0, max(ra[1], rb[1]))
            gb, nb = self.down(self.b, isp)
            count = _power_bounds(gb, nb, self.b.get_field(chargeden=False)["electric"], self.inp, which)
            for name in db:
                c = count[name]
                for key, n, scale in (("xv", c["count"], np.max(np.abs(db[name]["xv"]))),
                                      ("v", c["count"].sum(axis=1), np.max(np.abs(db[name]["v"]))),
                                      ("rest", c["rest"]["count"], c["rest"]["abs"])):
                    want = np.asarray(db[name][key])
                    tol = n * q + 1e-10 * scale + 2.0 * PR.U * np.abs(want)
                    assert np.all(np.abs(np.asarray(da[name][key]) - want) <= tol), \
                        ("power_local_exact a against b", name, key, self.tail())
        if not self.full:
            return
        refs = []
        for i, g, n, e in self.sources(isp):
            if i == 1 and self.exact:
                refs.append(refs[0])
                continue
            E = e.get_field(chargeden=False)["electric"]
            refs.append(PX.reference(*_cut(g, n), E, self.inp, which, isp))
        for got, ref, who in zip((ra, rb), refs, "ab"):
            assert got[1] == ref["e"], ("power_local_exact", who, "e", got[1], ref["e"], self.tail())
            assert got[0].dtype == np.int64 and np.array_equal(got[0], ref["limbs"]), ("power_local_exact", who, self.tail())

    def rule(self, args):
        lx = self.inp.lx
        return dict(x=(args["x"][0] * lx, args["x"][1] * lx), v=tuple(args["v"]), fraction=args["fraction"], key=args["key"], origin=0)

    def select_reference(self, args, g, n):
        r = self.rule(args)
        return SR.select(g, self.inp.lx, n=n, x_window=r["x"], v_window=r["v"], thin=SR.thin_of(r["fraction"]), key=r["key"], origin=0)

    def do_select(self, args):
        return lambda e: e.select(args["isp"], **self.rule(args))

    def check_select(self, args, ra, rb):
        for (i, g, n, _), got in zip(self.sources(args["isp"]), (ra, rb)):
            SR.assert_same(got, self.select_reference(args, g, n), what=("select", "ab"[i], self.tail()))
        if self.exact:
            SR.assert_same(ra, rb, what=("select a against b", self.tail()))

    def do_select_count(self, args):
        return lambda e: e.select_count(args["isp"], **self.rule(args))

    def check_select_count(self, args, ra, rb):
        for (i, g, n, _), got in zip(self.sources(args["isp"]), (ra, rb)):
            assert got == self.select_reference(args, g, n)["count"], ("select_count", "ab"[i], self.tail())

    def do_gather(self, args):
        return lambda e: e.gather(args["isp"], args["index"])

    def check_gather(self, args, ra, rb):
        idx = np.array(args["index"], dtype=np.int64)
        for (i, g, _, _), got in zip(self.sources(args["isp"]), (ra, rb)):
            for k in "xvpw":
                assert SR.same_bits(got[k], g[k][idx]), ("gather", "ab"[i], k, self.tail())

    def do_state_digest(self, args):
        return lambda e: e.state_digest()

    def check_state_digest(self, args, ra, rb):
        for isp in range(self.nsp):
            for (i, g, _, _), got in zip(self.sources(isp), (ra, rb)):
                want = [self.amd.host_digest(g[k]) for k in "xvwp"]          # (all nalloc slots)
                assert [int(d) for d in got[isp]] == want, ("state_digest", "ab"[i], isp, self.tail())

    def do_output_all(self, args):
        return lambda e: e.output_all()

    def check_output_all(self, args, ra, rb):
        for (scal, fld, dists), e, who in ((ra, self.a, "a"), (rb, self.b, "b")):
            # the separate calls on the same engine, with the tolerances of test_output_all_in_one_call_equals_the_separate_calls.
            # (They may be served from the very pass output_all cached: this holds the record together, not the numbers --
            # those are held by a against b below, bit for bit with the exact sums, and by the tests of the diagnostics.)
            # (where field_chargeden holds a half step's kept mode only, get_field(chargeden) would rebuild it: not asked for)
            want_fld = e.get_field(chargeden=not e.chargeden_kept_mode_only())
            for k in want_fld:
                scale = max(np.max(np.abs(want_fld[k])), 1e-300)
                assert np.max(np.abs(fld[k] - want_fld[k])) < 1e-11 * scale, ("output_all", who, k, self.tail())
            want_scal = e.output_scalars()
            tol = 1e-11 * np.abs(want_scal)
            for isp in range(self.nsp):     # the perturbed kinetic sum cancels heavily: against the scale of its terms
                tol[4 + 3 * isp] = max(tol[4 + 3 * isp], 1e-12 * abs(want_scal[3 + 3 * isp]))
            assert np.all(np.abs(scal - want_scal) <= tol), ("output_all", who, scal, want_scal, self.tail())
            for isp in range(self.nsp):
                want = e.ptcldist(isp)
                for k in want:
                    assert np.max(np.abs(dists[isp][k] - want[k])) <= 1e-11 * max(np.max(np.abs(want[k])), 1e-300), \
                        ("output_all", who, isp, k, self.tail())
        if self.exact:
            assert np.array_equal(ra[0], rb[0]), ("output_all a against b: scalars", self.tail())
            for k in FIELD_KEYS:
                assert np.array_equal(ra[1][k], rb[1][k]), ("output_all a against b", k, self.tail())
            for isp in range(self.nsp):
                for k in DIST_KEYS:
                    assert np.array_equal(ra[2][isp][k], rb[2][isp][k]), ("output_all a against b", isp, k, self.tail())
        else:
            for k in ("electric", "mode_re", "mode_im"):
                self.cmp.close(ra[1][k], rb[1][k], ("output_all a against b", k))
            if not self.a.chargeden_kept_mode_only():
                self.cmp.close(ra[1]["chargeden"], rb[1]["chargeden"], ("output_all a against b", "chargeden"))
            else:
                ka, kb = (_kept_coefficients(r[1]["chargeden"], self.seq["kw"]["modes"]) for r in (ra, rb))
                scale = max(np.max(np.abs(kb)), np.max(np.abs(rb[1]["chargeden"])), 1e-300)
                assert np.max(np.abs(ka - kb)) <= 1e-10 * scale, ("output_all a against b", "kept modes of chargeden", self.tail())

    # -- checkpoint and restart ------------------------------------------------------
    def checkpoint(self, args):
        at, expect = args["at"], args["expect"]
        self.nckpt += 1
        if expect == "refused":
            for e, who in ((self.a, "a"), (self.b, "b")):
                path = str(self.tmp / ("refused%d%s.ckpt" % (self.nckpt, who)))
                code, _ = self.bracket(e, lambda eng: eng.checkpoint_write(path), "refused checkpoint_write")
                assert code == ERR_STATE, ("checkpoint_write inside a time step", who, code, self.tail())
                assert not os.path.exists(path) and not os.path.exists(path + ".tmp"), (who, self.tail())
            self.ran[("checkpoint", at, "refused")] += 1
            return
        self.skips += self.a.kernel_stats(11)[1] - self.skips0
        fresh = []
        for e, who, like in ((self.a, "a", self.like_a), (self.b, "b", self.like_b)):
            path = str(self.tmp / ("run%d%s.ckpt" % (self.nckpt, who)))
            e.checkpoint_write(path)
            new = like(lambda: self.amd.Pic1dp.from_checkpoint(path))
            assert np.array_equal(new.state_digest(), e.state_digest()), ("restart: markers", who, self.tail())
            fo, fn = e.get_field(), new.get_field()
            for k in FIELD_KEYS:
                assert fo[k].tobytes() == fn[k].tobytes(), ("restart", who, k, self.tail())
            assert new.energy_history().tobytes() == e.energy_history().tobytes(), ("restart: history", who, self.tail())
            assert new.predict_kind() == e.predict_kind(), ("restart: configuration", who, self.tail())
            e.close()
            fresh.append(new)
        self.a, self.b = fresh
        self.cmp.a, self.cmp.b = fresh
        self.skips0 = self.a.kernel_stats(11)[1]
        self.ran[("checkpoint", at, "restart")] += 1

    # -- everything else ---------------------------------------------------------------
    def all3(self):
        return (self.a, self.b, self.c)

    def run(self):
        nx = self.inp.nx
        for op, args in self.seq["ops"]:
            if op in CS.READ_ONLY:
                self.read_only(op, args)
                continue
            self.log.append(op)
            if op in ("push1", "push2"):
                for e in self.all3():
                    e.interaction_push_particle(int(op[-1]))
            elif op == "collect":
                for e in self.all3():
                    e.interaction_collect_charge()
            elif op == "solve":
                for e in self.all3():
                    e.field_solve_electric()
            elif op == "pair-setup":            # the fused / predicted paths need the dense-table mode-filter solve
                for e in self.all3():
                    e.set_field_solver(0)
                    e.set_field_transform(0)
            elif op == "step":
                for e in self.all3():
                    e.step(args["n"])
            elif op in ("substep1", "substep2"):
                for e in self.all3():
                    e.substep(int(op[-1]))
            elif op == "setE":
                E = (0.02 * np.sin(2 * np.pi * np.arange(nx) / nx + args["phase"])
                     + 0.002 * np.random.default_rng(args["noise"]).standard_normal(nx))
                for e in self.all3():
                    e.set_electric(E)
            elif op == "setcd":
                cd = self.b.get_field()["chargeden"] * args["factor"]
                for e in self.all3():
                    e.set_chargeden(cd)
            elif op == "solver":
                for e in self.all3():
                    e.set_field_solver(args["kind"])
            elif op == "transform":
                for e in self.all3():
                    e.set_field_transform(args["kind"])
            elif op == "optimize":
                for e in self.all3():
                    e.particle_optimize(2)
            elif op == "upload":                # b's markers, into all
                for isp in range(self.nsp):
                    d, npv = self.down(self.b, isp)
                    for e in self.all3():
                        e.particles_upload(d["x"], d["v"], d["p"], d["w"], ispecies=isp, np_valid=npv)
            elif op == "download":              # a look, as the older differential has them (c takes it too)
                self.markers(self.cmp, op)
                self.cmp.field(op, False)
                for isp in range(self.nsp):
                    self.c.particles_download(isp)
                self.c.get_field(chargeden=False)
            elif op == "hostsum":               # a host that owns the reduction; the read-only intruders inside are at P
                local = [e.charge_local_exact() if self.exact else e.charge_local() for e in self.all3()]
                for k, a in args["inside"]:
                    self.read_only(k, a)
                self.log.append("charge_reduced")
                for e, q in zip(self.all3(), local):
                    e.charge_reduced_exact(q) if self.exact else e.charge_reduced(q)
            else:
                raise AssertionError("unknown op " + op)
        for tag in ("end", "end, looked again"):    # (a second look: what the first one settled stays settled)
            self.cmp.field(tag, True)
            self.markers(self.cmp, tag)
        self.cmp.history("end")
        self.skips += self.a.kernel_stats(11)[1] - self.skips0
        if self.seq["pair_case"]:
            assert self.skips >= 1, ("the pair path was never served", self.log)
        # c ran the sequence without the read-only intruders: what they left behind on a shows here
        cmp_c = _Compare(self.c, self.a, self.kind or 1, self.seq["kw"]["modes"], self.exact, self.log)
        self.field_by_both_flags(cmp_c, "c against a")
        self.markers(cmp_c, "c against a")
        cmp_c.history("c against a")
        for e in self.all3():
            e.close()
        return self.ran, self.skips


@pytest.mark.parametrize("seed", seeds(CS.DEFAULT_SEEDS["tiles"]))
def test_call_sequences_tiles(amd, monkeypatch, tmp_path, seed):
    """the prediction as tiles (PIC1DP_PRED_KIND=1): a against b and c against a within 1e-10"""
    ran, skips = _Run(amd, monkeypatch, tmp_path, "tiles", seed).run()
    print("intrusions:", dict(ran))


@pytest.mark.parametrize("seed", seeds(CS.DEFAULT_SEEDS["sums"]))
def test_call_sequences_sums(amd, monkeypatch, tmp_path, seed):
    """the prediction as six sums (PIC1DP_PRED_KIND=2), mostly one kept mode on one rank with two quiet stretches so that the
    pair path is served (kernel_stats(11) skips >= 1) and meets a read-only intruder behind its collect_charge (HalfPair,
    AdoptHalfField owed) and behind its solve_field (HalfPairSolved)"""
    ran, skips = _Run(amd, monkeypatch, tmp_path, "sums", seed).run()
    print("intrusions:", dict(ran), "pair skips:", skips)


@pytest.mark.parametrize("seed", seeds(CS.DEFAULT_SEEDS["exact"]))
def test_call_sequences_exact(amd, monkeypatch, tmp_path, seed):
    """set_charge_sum(1) and set_diag_sum(1) on every engine right after the load: a against b, the restored contexts and c
    against a bit for bit"""
    ran, skips = _Run(amd, monkeypatch, tmp_path, "exact", seed).run()
    print("intrusions:", dict(ran))


@pytest.mark.parametrize("sites", ["lazy", "eager"])
def test_checkpoint_write_is_refused_after_each_of_the_first_five_calls(amd, monkeypatch, tmp_path, sites):
    """(found by the sequences above -- every seed whose refused checkpoint met engine b, the shortest `push1, checkpoint@B1`;
    on engine a `push1, collect, solve, push2, collect, checkpoint@B5`.)  pic1dp_hip_checkpoint_write told "inside a time
    step" by a NOTED push alone: eager call sites note none, so after push(1) they wrote a file that carries no RK backup
    for the push(2) to come and put the context into the state of a restart in the middle of its step; lazy call sites have
    nothing noted behind the second collect_charge and wrote there, with the solve of the new state outstanding.  The call
    record (call_phase) decides now, alike for both: refused after each of the first five of the six calls, after
    substep(1), and with a charge_local pending; served between time steps, also where step, substep(2) or an upload ended
    the time step early."""
    if sites == "eager":
        monkeypatch.setenv("PIC1DP_LAZY_CALLS", "0")
        monkeypatch.setenv("PIC1DP_PREDICT", "0")
    e = Checked(amd.Pic1dp(amd.make_input(nparticle_max=20001, nx=48)))
    e.particle_load()
    e.interaction_collect_charge()
    e.field_solve_electric()
    e.step(2)
    count = [0]

    def write(served):
        count[0] += 1
        path = str(tmp_path / ("w%d.ckpt" % count[0]))
        d0 = e.state_digest()
        if served:
            e.checkpoint_write(path)
            assert amd.checkpoint_info(path)["digest"] == [[int(v) for v in row] for row in d0]
        else:
            with pytest.raises(amd.Pic1dpError) as ei:
                e.checkpoint_write(path)
            assert ei.value.code == ERR_STATE, str(ei.value)
            assert not os.path.exists(path) and not os.path.exists(path + ".tmp")
            e.check_state(True)
        assert np.array_equal(e.state_digest(), d0)

    six = [lambda: e.interaction_push_particle(1), e.interaction_collect_charge, e.field_solve_electric,
           lambda: e.interaction_push_particle(2), e.interaction_collect_charge, e.field_solve_electric]
    write(True)
    for i, call in enumerate(six):
        call()
        write(i == 5)
    e.substep(1)
    write(False)
    e.substep(2)
    write(True)
    e.interaction_push_particle(1)
    e.interaction_collect_charge()
    e.interaction_collect_charge()              # (a second collect_charge of the same sub-step moves nothing on)
    write(False)
    e.step(1)                                   # a whole step ends the one the host had begun
    write(True)
    e.interaction_push_particle(1)
    q = e.charge_local()
    write(False)
    e.charge_reduced(q)
    e.field_solve_electric()
    e.interaction_push_particle(2)
    e.charge_reduced(e.charge_local())
    write(False)                                # the fifth call, made by the host's own reduction
    e.field_solve_electric()
    write(True)
    e.close()
