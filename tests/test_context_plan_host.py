"""What pic1dp_hip_create decides before its first allocation (pic1dp_amd/csrc/context_plan.cpp plan_context) against a
table recorded from create()'s own formulas as they were before they became a pure function
(tests/golden/gen_context_plan.py), and what it takes from the environment (settings.cpp settings_from_env).  No GPU."""
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def probe():
    from pic1dp_amd import probe as p
    p.load()
    return p


@pytest.fixture(scope="module")
def table():
    """the recorded table, its rows [query, plan] as dicts; sc_re / sc_im are recorded once per grid"""
    t = json.load(open(os.path.join(ROOT, "tests", "golden", "context_plan.json")))
    sc = dict(zip(t["nx"], t["sc"]))
    rows = []
    for q, p in t["rows"]:
        q, p = dict(zip(t["query"], q)), dict(zip(t["plan"], p))
        p["sc_re"], p["sc_im"] = sc[q["nx"]]
        rows.append({"query": q, "plan": p})
    return dict(t, rows=rows)


def ask(probe, table, nx, nm, ns, pred_req=0, gcopies_req=0, layout=(1, 0, 0), one_rank_order=0, opt=(0, 0, 0)):
    import pic1dp_amd
    inp = pic1dp_amd.make_input(nx=nx, nmode=nm, modes=list(range(1, nm + 1)), nspecies=ns, nparticle_max=table["nparticle_max"],
                                species_nparticle_init=table["nparticle_init"][:ns], species_charge=[-1.0, 1.0][:ns],
                                species_mass=[1.0, 2.0][:ns], nmerge=opt[0], nremove=opt[1], nsplit=opt[2])
    nranks, npe, rank = layout
    return probe.host_context_plan(inp, nranks=nranks, npe=npe, rank=rank, pred_kind_req=pred_req, gcopies_req=gcopies_req,
                                   one_rank_order=one_rank_order)


def test_every_plan_is_the_recorded_one(probe, table):
    """Every field of the plan -- blocks and slots, accumulator copies, the one-pass kernel and its buffers' sizes, the
    field's table staging, summation order and scales, the optimisation counters -- on the turning points: nx 1, 7 | 8
    (the six sums need nx >= 8), 192, 256 | 257 (eight accumulator copies | one), 1024, 1096 | 1097 (the private slots of
    two workgroups fit a CU | do not), the largest nx on either side of where the tiles of 1, 2 and 3 kept modes and the
    six sums outgrow the LDS; 1 ... 4 kept modes (the tiles serve three); one and two species; PIC1DP_PRED_KIND none, 1, 2,
    3; PIC1DP_RHO_GLOBAL_COPIES none, 4, 3 and 128 (both refused); one rank, one rank of eight reference blocks, the second
    of two ranks with four blocks each, the last of eight -- of a marker count that divides by neither 2 nor 8."""
    t = table
    assert {1, 7, 8, 192, 256, 257, 1024, 1096, 1097} <= set(t["nx"]) and len(t["nx"]) == 9 + 8
    assert t["nparticle_max"] % 8 != 0 and t["nparticle_max"] % 2 != 0
    seen = {"pred": set(), "req": set(), "gcopies_req": set(), "layout": set(), "nm": set(), "ns": set(), "nx": set()}
    for row in t["rows"]:
        q, want = row["query"], row["plan"]
        got = ask(probe, t, **q)
        assert set(got) == set(want)
        bad = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
        if bad:
            pytest.fail("%r: (got, recorded) %r" % (q, bad))
        seen["pred"].add((got["pred_kind"], got["pred_private"]))
        seen["req"].add(q.get("pred_req", 0)), seen["gcopies_req"].add(q.get("gcopies_req", 0))
        seen["layout"].add(tuple(q.get("layout", (1, 0, 0)))), seen["nm"].add(q["nm"]), seen["ns"].add(q["ns"]), seen["nx"].add(q["nx"])
    assert seen["pred"] == {(0, 0), (1, 0), (2, 0), (2, 1)}      # two passes, tiles, register sums, private sums
    assert seen["req"] == {0, 1, 2, 3} and seen["gcopies_req"] == {0, 4, 3, 128}
    assert seen["layout"] == {(1, 0, 0), (1, 8, 0), (2, 8, 1), (8, 8, 7)}
    assert seen["nm"] == {1, 2, 3, 4} and seen["ns"] == {1, 2} and seen["nx"] == set(t["nx"])


def test_the_table_sits_on_the_turning_points(table):
    """the recorded plans change where they should: between the neighbouring grids of every threshold"""
    rows = {json.dumps(r["query"], sort_keys=True): r["plan"] for r in table["rows"]}
    full = dict(pred_req=0, gcopies_req=0, layout=[1, 0, 0], one_rank_order=0, opt=[0, 0, 0])
    plan = lambda **q: rows[json.dumps(dict(full, **q), sort_keys=True)]
    nxs = table["nx"]
    extra = [n for n in nxs if n not in (1, 7, 8, 192, 256, 257, 1024, 1096, 1097)]
    assert len(extra) == 8 and all(b == a + 1 for a, b in zip(extra[::2], extra[1::2]))
    # three kept modes outgrow the LDS first, then two, then one; the six sums last
    (t3, _), (t2, _), (t1, _), (s1, _) = [(extra[i], extra[i + 1]) for i in range(0, 8, 2)]
    for nm, last in ((3, t3), (2, t2)):
        assert plan(nx=last, nm=nm, ns=1, pred_req=0)["pred_kind"] == 1 and plan(nx=last + 1, nm=nm, ns=1, pred_req=0)["pred_kind"] == 0
    assert plan(nx=t1, nm=1, ns=1, pred_req=1)["pred_kind"] == 1 and plan(nx=t1 + 1, nm=1, ns=1, pred_req=1)["pred_kind"] == 2
    assert plan(nx=s1, nm=1, ns=1, pred_req=0)["pred_kind"] == 2 and plan(nx=s1 + 1, nm=1, ns=1, pred_req=0)["pred_kind"] == 0
    assert t3 < t2 < t1 < s1
    assert plan(nx=256, nm=1, ns=1, gcopies_req=0)["gcopies"] == 8 and plan(nx=257, nm=1, ns=1, gcopies_req=0)["gcopies"] == 1
    assert [plan(nx=257, nm=1, ns=1, gcopies_req=g)["gcopies"] for g in (4, 3, 128)] == [4, 1, 1]
    p = plan(nx=192, nm=1, ns=2, layout=[2, 8, 1], one_rank_order=0, opt=[0, 0, 0])
    assert len(set(p["blk_alloc"])) == 2 and p["blk0"] == 4 and p["nblk"] == 4 and p["np"][1] < p["np"][0] == p["nalloc"]
    assert plan(nx=192, nm=1, ns=2, layout=[2, 8, 1], one_rank_order=1, opt=[0, 0, 0])["field_npe"] == 1 and p["field_npe"] == 8
    assert plan(nx=192, nm=1, ns=1, layout=[1, 0, 0], one_rank_order=0, opt=[2, 0, 1])["imerge"] == 1


@pytest.mark.parametrize("nx,force,kind", [(8, 0, 2), (7, 0, 1), (192, 0, 2), (192, 1, 1), (1096, 0, 2), (1097, 0, 1), (1097, 2, 2)],
                         ids=["private_first", "below", "default_grid", "default_grid_forced_tiles", "private_last", "beyond_default",
                              "beyond_forced_sums"])
def test_private_sums_at_their_limits_on_the_host(probe, table, nx, force, kind):
    """the seven choices tests/test_gpu_one_pass.py::test_private_sums_at_their_limits observes on a GPU, from the table
    and from the library"""
    want = [r["plan"] for r in table["rows"] if r["query"] == dict(nx=nx, nm=1, ns=1, pred_req=force, gcopies_req=0, layout=[1, 0, 0],
                                                                 one_rank_order=0, opt=[0, 0, 0])]
    assert want and all(w == want[0] for w in want) and want[0]["pred_kind"] == kind
    got = ask(probe, table, nx, 1, 1, pred_req=force)
    assert got["pred_kind"] == kind
    # k_step_one<PRIV> wherever the six sums were not insisted on and the slots fit (nx <= 1096)
    assert got["pred_private"] == (1 if kind == 2 and nx <= 1096 else 0)


PRODUCT_ENV = ["PIC1DP_FUSE_SOLVE", "PIC1DP_TAIL", "PIC1DP_CALL_PAIR", "PIC1DP_LAZY_CALLS", "PIC1DP_PREDICT", "PIC1DP_DIAG_FX",
               "PIC1DP_DIAG_FX_MARGIN", "PIC1DP_PRED_KIND", "PIC1DP_CHAIN_MFMA"]
TUNING_ENV = ["PIC1DP_OSUB", "PIC1DP_DYN_TAIL", "PIC1DP_DYN_TAIL_FULL", "PIC1DP_NT_THRESHOLD_MB", "PIC1DP_NT_THRESHOLD_FULL_MB",
              "PIC1DP_CARRY", "PIC1DP_RHO_GLOBAL_COPIES", "PIC1DP_FIELD_ONE_RANK_ORDER", "PIC1DP_CHAIN_SELFTEST_VERBOSE"]
DEFAULTS = dict(fuse_solve=1, tail_on=1, call_pair=1, lazy_calls=1, predict=1, carry=-1, osub_req=0, dyn_tail=8, dyn_tail_full=16,
                diag_fx=1, pred_kind_req=0, chain_mfma_req=-1, gcopies_req=0, field_one_rank_order=0, chain_selftest_verbose=0,
                nt_threshold_half=2048.0 * 1048576.0, nt_threshold_full=288.0 * 1048576.0, diag_fx_margin_w=16.0)


@pytest.fixture
def clean_env(monkeypatch):
    for name in PRODUCT_ENV + TUNING_ENV:
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


def test_settings_defaults(probe, clean_env):
    assert probe.host_settings() == DEFAULTS


def test_settings_clamps_and_precedence(probe, clean_env):
    env = clean_env
    for given, taken in (("7", 2), ("-1", 0), ("0", 0), ("1", 1), ("2", 2)):
        env.setenv("PIC1DP_FUSE_SOLVE", given)
        assert probe.host_settings()["fuse_solve"] == taken
    for name, field in (("PIC1DP_TAIL", "tail_on"), ("PIC1DP_CALL_PAIR", "call_pair"), ("PIC1DP_LAZY_CALLS", "lazy_calls"),
                        ("PIC1DP_DIAG_FX", "diag_fx")):
        env.setenv(name, "0")
        assert probe.host_settings()[field] == 0
        env.setenv(name, "2")
        assert probe.host_settings()[field] == 1
    for given in ("0", "1", "5", "-3"):      # taken as given
        env.setenv("PIC1DP_PREDICT", given)
        assert probe.host_settings()["predict"] == int(given)
    env.setenv("PIC1DP_DIAG_FX_MARGIN", "1.25")
    assert probe.host_settings()["diag_fx_margin_w"] == 1.25
    for given in ("1", "2", "3", "9"):       # a request: context_plan.cpp decides what it can serve
        env.setenv("PIC1DP_PRED_KIND", given)
        assert probe.host_settings()["pred_kind_req"] == int(given)
    for given, taken in (("0", 0), ("1", 1), ("4", 1), ("-1", -1)):   # unset / 0 / positive
        env.setenv("PIC1DP_CHAIN_MFMA", given)
        assert probe.host_settings()["chain_mfma_req"] == taken
    # every other field kept its default through all of this
    got = probe.host_settings()
    touched = {"fuse_solve", "tail_on", "call_pair", "lazy_calls", "diag_fx", "predict", "diag_fx_margin_w", "pred_kind_req", "chain_mfma_req"}
    assert {k: v for k, v in got.items() if k not in touched} == {k: v for k, v in DEFAULTS.items() if k not in touched}


def test_tuning_variables_change_nothing_in_the_product_build(probe, clean_env):
    """the probe library is a product build: tuning_env() looks at nothing (kernels.hpp)"""
    for name in TUNING_ENV:
        clean_env.setenv(name, "3")
    assert probe.host_settings() == DEFAULTS


def test_mode_tables_equal_the_loops_create_held_bit_for_bit(tmp_path):
    """tests/mode_tables_check.cpp, a program of its own: mode_tables() against a literal copy of create()'s former loops, as
    bytes, for nx 7, 192, 1024 and kept modes {1}, {1, 2, 3} -- built with context_plan.cpp and settings.cpp under
    AddressSanitizer and UndefinedBehaviorSanitizer (host code only; nothing of it touches a GPU), with the product's
    floating-point flags"""
    import importlib.util
    import subprocess
    spec = importlib.util.spec_from_file_location("pic1dp_amd_build", os.path.join(ROOT, "pic1dp_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    csrc = os.path.join(ROOT, "pic1dp_amd", "csrc")
    exe = str(tmp_path / "mode_tables_check")
    subprocess.check_call([build.hipcc(), "--offload-arch=gfx950", "-x", "hip", "--offload-host-only", "-O3", "-g", "-std=c++17",
                           "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "mode_tables_check.cpp")] +
                          [os.path.join(csrc, f) for f in ("context_plan.cpp", "settings.cpp", "loader.cpp", "multirand.cpp")] +
                          ["-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("15 cases, 0 differ"), r.stdout
