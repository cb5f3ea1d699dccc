"""bench.py end to end on the GPU box: the default contract line on one rank, and
rehearsals of the multi-rank control flow -- two ranks launched by
torch.distributed.run sharing the one GPU (RCCL needs one GPU per rank, so the charge
is summed by the library's one-hop exchange through IPC-mapped memory, or host-staged
through gloo) -- for the configurations c3, c4 and c5 of BASELINE.json, whose physics
must equal a one-process run holding the same reference rank blocks as virtual ranks."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def bench_module():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_bench(args, nproc=1, timeout=900, port=29533, self_launch=False):
    """nproc > 1: under torch.distributed.run (the contract's launch line), or -- self_launch -- as the plain
    `python bench.py --gpus N ...` the driver uses, which starts its own rank processes"""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0", PIC1DP_XCHG_TIMEOUT_MS="60000")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    if nproc == 1 or self_launch:
        cmd = [sys.executable, os.path.join(ROOT, "bench.py")] + args
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc),
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py")] + args
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


CONTRACT_KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                 "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "attribution", "strong_1e8_total")


@pytest.mark.parametrize("config,nx,kernel,carry", [("c3", 256, "k_step_one<sums>", 0.0), ("c3", 1024, "k_step_one<sums>", 0.0),
                                                    ("c5", 4096, "k_step_sums", 0.0)])
def test_bench_contract_line_small(config, nx, kernel, carry):
    """the one JSON line of a --full run (N = 1), without the traffic passes: contract keys, the roofline
    priced on the bytes the LIBRARY reports for the instantiation it launched (pic1dp_hip_kernel_bytes), and the
    same launch priced on the compulsory bytes alone (frac_compulsory)"""
    n = 2_000_000
    d = run_bench(["--config", config, "--particles", str(n), "--strong-total", str(n), "--nx", str(nx), "--steps", "5",
                   "--warmup", "2", "--repeats", "5", "--full", "--no-cpu-baseline", "--no-traffic-pass"])
    for key in CONTRACT_KEYS:
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 5 and d["warmup"] == 2 and d["dtype"] == "f64"
    assert d["warmup_effective"] == d["warmup"] + d["settle_steps_before_warmup"]
    assert d["vs_baseline"] is None and d["scaling"] == "weak" and d["higher_is_better"] is True
    assert abs(d["value"] - n * 2 * 5 / (d["ms_per_step"] * 5e-3)) < 1e-6 * d["value"]
    # --repeats R: the timed block of K steps is run R >= 5 times back to back: the line carries the median block and the spread
    assert d["repeats"] >= 5 and len(d["ms_per_step_blocks"]) == d["repeats"]
    assert d["ms_per_step_min"] <= d["ms_per_step"] <= d["ms_per_step_max"]
    assert d["ms_per_step"] == sorted(d["ms_per_step_blocks"])[(d["repeats"] - 1) // 2]
    assert d["config"]["timed_blocks"] == d["repeats"]
    assert sum(d["config"]["kernel_launches_in_timed_steps"].values()) == d["repeats"] * d["steps"]
    assert d["steps_before_field_energy_end"] == d["warmup_effective"] + d["repeats"] * d["steps"]
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["peak"] == 8000.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12
    assert kernel in r["kernel"] and "pic1dp_hip_kernel_bytes" in r["bytes_per_marker_source"]
    assert kernel in r["bytes_per_marker_source"]
    # compulsory: 32 B read (x, v, w, p) + 24 B written (x, v, w) per marker and launch (= time step); what the
    # kernel moves beyond that is the carry of -f0'/f0 it chooses (0 for the Maxwellian of c5)
    assert r["bytes_compulsory"] == 56.0 and r["bytes_per_marker"] in (56.0, 72.0)
    if carry is not None:
        assert r["bytes_per_marker"] == 56.0 + carry
    assert abs(r["achieved"] - r["bytes_per_marker"] * n / (r["avg_launch_ms"] * 1e-3) / 1e9) < 1e-6 * r["achieved"]
    assert abs(r["frac_compulsory"] - 56.0 * n / (r["avg_launch_ms"] * 1e-3) / 1e9 / 8000.0) < 1e-9
    assert r["frac_compulsory"] <= r["frac"]
    assert abs(r["reference_priced_GBs"] / r["achieved"] - 160.0 / r["bytes_per_marker"]) < 1e-9
    assert r["whole_step_bytes"] == r["bytes_per_marker"] * n          # every timed step was one launch
    assert r["whole_step_GBs"] <= r["peak"]
    assert r["traffic"] is None or "not measured in this run" in r["traffic_source"]
    assert d["strong_1e8_total"]["same_run_as_headline"] is True
    assert d["drop_in_call_sites"]["value"] > 0
    assert d["attribution"]["particle_kernels_ms_per_step"] > 0 and d["attribution"]["field_solve_ms_per_step"] > 0


def test_bench_measures_its_own_traffic():
    """roofline.traffic measured for this very command by two child `rocprofv3 --pmc` passes: the bytes the
    kernel has to move plus the tiles' staging and flush (small at any realistic marker count)"""
    import shutil
    if shutil.which("rocprofv3") is None and not os.path.exists("/opt/rocm/bin/rocprofv3"):
        pytest.skip("rocprofv3 not installed")
    n = 8_000_000
    d = run_bench(["--particles", str(n), "--strong-total", str(n), "--nx", "256", "--steps", "5", "--warmup", "2",
                   "--full", "--no-cpu-baseline"])
    r = d["roofline"]
    if r["traffic"] is None or "measured for this command in this run" not in (r["traffic_source"] or ""):
        pytest.skip("the counter passes were not possible here: %s" % r["traffic_source"])
    assert 0.97 < r["traffic"] / (r["bytes_per_marker"] * n) < 1.25


def test_bench_dumps_what_its_last_timed_step_computed(amd, tmp_path):
    """--dump-outputs DIR after K timed steps (--steps K, one block by default): the field and a seeded sample of the
    markers are those of one engine stepped as often on the same input"""
    import numpy as np
    b = bench_module()
    n, steps = 2_000_000, 5
    d = run_bench(["--particles", str(n), "--strong-total", str(n), "--nx", "256", "--steps", str(steps), "--warmup", "2",
                   "--no-cpu-baseline", "--no-traffic-pass", "--dump-outputs", str(tmp_path / "out")])
    assert d["repeats"] == 1 and sum(d["config"]["kernel_launches_in_timed_steps"].values()) == steps
    after = d["dumped_outputs"]["after_steps"]
    assert after == d["warmup_effective"] + steps == d["steps_before_field_energy_end"]
    got = {k: np.load(str(tmp_path / "out" / (k + ".npy"))) for k in d["dumped_outputs"]["names"]}
    assert sorted(got) == ["chargeden", "electric", "field_energy", "mode_im", "mode_re", "p", "v", "w", "x"]
    assert all(a.dtype == np.float64 for a in got.values()) and sum(a.nbytes for a in got.values()) <= 64 << 20
    eng = amd.Pic1dp(amd.make_input(nparticle_max=n, nx=256))
    eng.particle_load()
    eng.interaction_collect_charge()
    eng.field_solve_electric()
    eng.step(after)
    assert abs(float(got["field_energy"][0]) / eng.field_energy() - 1.0) < 1e-10
    f = eng.get_field()
    for k in ("electric", "chargeden"):
        assert np.max(np.abs(got[k] - f[k])) <= 1e-10 * np.max(np.abs(f[k])), k
    _, np_valid = eng.local_sizes()
    idx = b.dump_sample(np_valid, 0, 1)
    assert len(idx) == len(got["x"]) == b.DUMP_MARKERS
    ref = eng.particles_download()
    assert np.array_equal(got["p"], ref["p"][idx])
    assert np.max(np.abs(got["x"] - ref["x"][idx])) < 1e-9 and np.max(np.abs(got["v"] - ref["v"][idx])) < 1e-9
    eng.close()


def virtual_rank_energy(amd, kw, npe, nsteps):
    eng = amd.Pic1dp(amd.make_input(**kw), npe=npe)
    eng.particle_load()
    eng.interaction_collect_charge()
    eng.field_solve_electric()
    eng.step(nsteps)
    return eng.field_energy()


@pytest.mark.parametrize("config,particles,allreduce,self_launch", [
    ("c3", 1_500_000, "p2p", False), ("c4", 3_000_000, "p2p", False), ("c5", 1_500_000, "p2p", False),
    ("c3", 1_000_000, "host", False), ("c3", 1_200_000, "auto", False),
    # the driver's own command form, `python3 bench.py --gpus N --steps K --warmup W`: no torchrun in the command
    ("c3", 1_100_000, "p2p", True), ("c5", 1_300_000, "auto", True)])
def test_bench_two_ranks_share_the_gpu(amd, config, particles, allreduce, self_launch):
    """the weak headline and the strong object, both present, both with the physics of the
    virtual-rank run (src/pic1dp_interaction.F90:126-150; `make run` uses 4 ranks, Makefile:39)"""
    b = bench_module()
    cfg = b.CONFIGS[config]
    phys = dict(cfg["inp"])
    nx_small = {"c3": 128, "c4": 128, "c5": 256}[config]
    phys["nx"] = nx_small
    steps, warm, strong_total = 6, 2, 2_000_000
    d = run_bench(["--gpus", "2", "--config", config, "--particles", str(particles), "--nx", str(nx_small),
                   "--steps", str(steps), "--warmup", str(warm), "--strong-total", str(strong_total),
                   "--allreduce", allreduce, "--full", "--no-cpu-baseline"], nproc=2, self_launch=self_launch)
    strong_cfg = "total" in cfg
    # round 6: on several ranks the metric's own configuration (c3) is measured STRONG-scaled -- `value` is the 10^8 (here:
    # --strong-total) markers in total, what north_star's ">= 6x from 1 -> 8" is a statement about --, the weak reading
    # (--particles per GPU) beside it as weak_per_gpu; c5 stays weak with the strong object beside it, c4 is strong by definition
    headline_strong = config == "c3"
    total = particles if strong_cfg else (strong_total if headline_strong else 2 * particles)
    assert d["n_gpus"] == 2 and d["config"]["particles_total"] == total
    assert d["scaling"] == ("strong" if (strong_cfg or headline_strong) else "weak")
    assert ("STRONG" in d["speedup_basis"]) == headline_strong
    assert ("IN TOTAL" in d["config"]["workload"]) == (strong_cfg or headline_strong)
    # auto: RCCL cannot put two ranks on one GPU, every rank agrees on the exchange instead
    assert d["config"]["allreduce"].startswith("host-staged" if allreduce == "host" else "one-hop")
    assert "allreduce_ms_per_step" in d["attribution"] and "field_solve_ms_per_step" in d["attribution"]
    at = d["attribution"]
    assert at["charge_sum"] == d["config"]["allreduce"] and set(d["config"]["charge_sum_not_used_because"]) == {"rccl", "one-hop exchange"}
    if allreduce != "host":
        # the exchange runs inside the field solve's launch: its share is read from a clock in the kernel, two a step
        # (one per charge sum ... a one-pass step sends both sums in ONE exchange)
        assert 0 < at["exchange_inside_field_launch_ms_per_step"] <= at["field_solve_ms_per_step"]
        assert at["exchanges_per_step"] >= 1 and at["allreduce_ms_per_step"] == 0
    nsteps = d["steps_before_field_energy_end"]
    assert nsteps == d["warmup_effective"] + d["repeats"] * steps
    e = virtual_rank_energy(amd, dict(nparticle_max=total, **phys), 2, nsteps)
    assert abs(d["field_energy_end"] / e - 1.0) < 1e-10
    if allreduce == "host":
        # the exchange measured beside another headline sum (on the driver's node: beside RCCL): both
        # workloads, with the physics of the headline run continued
        x = d["exchange"]
        assert x["weak"]["value"] > 0 and x["strong_1e8_total"]["value"] > 0
        assert "field_solve_ms_per_step" in x["weak"]["attribution"]
        # the strong figure is the one measured with the headline's charge sum; the exchange is listed beside it,
        # never promoted
        by = d["strong_1e8_total"]["by_charge_sum"]
        assert set(by) == {d["config"]["allreduce"], "one-hop exchange"}
        assert d["strong_1e8_total"]["value"] == by[d["config"]["allreduce"]]["value"]
        assert d["strong_1e8_total"]["allreduce"] == d["config"]["allreduce"]
    else:
        assert "exchange" not in d
    if strong_cfg:
        assert "strong_1e8_total" not in d and "weak_per_gpu" not in d      # the headline is the strong run itself
    elif headline_strong:
        s, w = d["strong_1e8_total"], d["weak_per_gpu"]
        assert s["same_run_as_headline"] is True and s["value"] == d["value"] and s["particles_total"] == strong_total
        assert w["particles_total"] == 2 * particles and w["particles_per_gpu"] == particles and w["scaling"] == "weak"
        assert w["same_run_as_headline"] is False and w["value"] > 0 and w["allreduce"] == d["config"]["allreduce"]
        e = virtual_rank_energy(amd, dict(nparticle_max=2 * particles, **phys), 2, nsteps)
        assert abs(w["field_energy_end"] / e - 1.0) < 1e-10
    else:
        s = d["strong_1e8_total"]
        assert s["particles_total"] == strong_total and s["same_run_as_headline"] is False and s["value"] > 0
        e = virtual_rank_energy(amd, dict(nparticle_max=strong_total, **phys), 2, nsteps)
        assert abs(s["field_energy_end"] / e - 1.0) < 1e-10


def test_bench_auto_chooses_the_charge_sum_by_rehearsal(amd):
    """with several kinds of charge sum up, `--allreduce auto` steps a scratch job of the
    strong-scaling share's size with each and takes the one whose step is shorter (max over ranks), saying so in
    config.charge_sum_chosen_by.  On a multi-GPU node the kinds are RCCL and the one-hop exchange; two ranks sharing this
    box's GPU cannot run RCCL, so the test lets the host-staged sum stand in as the second kind (--rehearse-with-host):
    the same code path, the same collective decisions."""
    d = run_bench(["--gpus", "2", "--config", "c3", "--particles", "600000", "--nx", "128", "--steps", "4", "--warmup", "2",
                   "--strong-total", "800000", "--allreduce", "auto", "--rehearse-with-host", "--no-cpu-baseline"],
                  nproc=2, self_launch=True)
    r = d["config"]["charge_sum_chosen_by"]
    assert set(r["ms_per_step"]) == {"p2p", "host"} and not r["failed"]
    assert all(v > 0 for v in r["ms_per_step"].values())
    assert r["chosen"] == min(r["ms_per_step"], key=r["ms_per_step"].get) and r["chosen"] in r["why"]
    assert d["config"]["allreduce"].startswith("one-hop" if r["chosen"] == "p2p" else "host-staged")
    assert r["markers_total"] == 800000
    # and without a second kind there is nothing to rehearse: the one that came up is taken
    d = run_bench(["--gpus", "2", "--config", "c3", "--particles", "600000", "--nx", "128", "--steps", "4", "--warmup", "2",
                   "--strong-total", "800000", "--allreduce", "auto", "--no-cpu-baseline"], nproc=2, self_launch=True)
    r = d["config"]["charge_sum_chosen_by"]
    assert r["chosen"] is None and "nothing to choose" in r["why"] and d["config"]["allreduce"].startswith("one-hop")


def test_bench_four_ranks_rehearsal_with_the_baseline_multi_gpu_configs(amd):
    """the driver's plain command at the reference's own rank count (`mpiexec -n 4`, Makefile:39 /
    run/Makefile:41) -- `python bench.py --gpus 4` started as ONE process, four rank processes sharing the box's GPU (with
    this test's own process five of the six the box admits on its card: `--gpus 8` as eight processes cannot run here),
    `--allreduce auto` choosing the charge sum by rehearsal (the host-staged sum standing in for RCCL), ONE JSON line whose
    `value` is the strong-scaling figure, the weak one beside it, and -- N = 4 -- BASELINE configs[3] measured as
    `configs3_c4`; configs[4] (`configs4_c5`, what --gpus 8 adds by itself) insisted on here.  Physics of every object
    against one engine holding the same four reference blocks as virtual ranks."""
    b = bench_module()
    steps, particles, strong_total, xp, xsteps = 4, 500_000, 1_200_000, 400_000, 3
    d = run_bench(["--gpus", "4", "--particles", str(particles), "--nx", "128", "--steps", str(steps), "--warmup", "2",
                   "--strong-total", str(strong_total), "--allreduce", "auto", "--rehearse-with-host", "--full", "--no-cpu-baseline",
                   "--extra-configs", "c4,c5", "--extra-particles", str(xp), "--extra-steps", str(xsteps)],
                  nproc=4, self_launch=True)
    assert d["n_gpus"] == 4 and d["scaling"] == "strong" and d["config"]["particles_total"] == strong_total
    r = d["config"]["charge_sum_chosen_by"]
    assert set(r["ms_per_step"]) == {"p2p", "host"} and not r["failed"] and r["chosen"] in ("p2p", "host")
    assert d["config"]["allreduce"].startswith("one-hop" if r["chosen"] == "p2p" else "host-staged")
    assert d["weak_per_gpu"]["particles_total"] == 4 * particles and d["weak_per_gpu"]["value"] > 0
    nsteps = d["steps_before_field_energy_end"]
    e = virtual_rank_energy(amd, dict(nparticle_max=strong_total, nx=128), 4, nsteps)
    assert abs(d["field_energy_end"] / e - 1.0) < 1e-10
    for key, name in (("configs3_c4", "c4"), ("configs4_c5", "c5")):
        x, cfg = d[key], b.CONFIGS[name]
        strong_x = "total" in cfg
        tot = xp if strong_x else 4 * xp
        assert x["particles_total"] == tot and x["scaling"] == ("strong" if strong_x else "weak") and x["nx"] == cfg["inp"]["nx"]
        assert x["value"] > 0 and x["steps"] == xsteps and len(x["ms_per_step_blocks"]) == 3
        assert x["allreduce"] == d["config"]["allreduce"] and x["attribution"]["particle_kernels_ms_per_step"] > 0
        assert "configs[%d]" % cfg["index"] in x["what"]
        e = virtual_rank_energy(amd, dict(nparticle_max=tot, **cfg["inp"]), 4, x["steps_before_field_energy_end"])
        assert abs(x["field_energy_end"] / e - 1.0) < 1e-10
    # without --extra-configs the rule is: c4 at N = 4, c5 at N = 8, nothing otherwise
    d2 = run_bench(["--gpus", "2", "--particles", "400000", "--nx", "128", "--steps", "3", "--warmup", "2", "--strong-total",
                    "600000", "--allreduce", "p2p", "--full", "--no-cpu-baseline"], nproc=2, self_launch=True)
    assert not any(k.startswith("configs") for k in d2)
