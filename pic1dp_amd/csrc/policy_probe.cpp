// policy_probe.cpp -- the launch policy (launch_policy.hpp) behind the C ABI of the probe library, for the host test that
// pins every shape (tests/test_launch_policy_host.py).  Test support (libpic1dp_probe.so), no GPU needed.
#include "../../include/pic1dp_probe.h"
#include "launch_policy.hpp"

using namespace pic1dp;

extern "C" int pic1dp_probe_host_launch_shape(const pic1dp_probe_launch_query *q, int64_t shape[4]) {
  if (!q || !shape) return 1;
  const LaunchPolicy p{q->num_cu, q->threads_req, q->bpc_req, q->osub_req};
  PredLaunch pl{};
  switch (q->family) {
    case 0: pl.lc = particle_launch(p, q->nx, q->np, q->with_E != 0, q->with_rho != 0, q->exact != 0); break;
    case 1: pl.lc = step_launch(p, q->nx, q->np, q->full != 0, q->exact != 0); break;
    case 2: pl.lc = step_diag_launch(p, q->nx, q->np, q->exact != 0, q->nx_opd, q->nv_opd); break;
    case 3: pl = pred_launch(p, q->nx, q->nmode, q->np, q->priv != 0, q->pred_kind, q->exp_bearing != 0); break;
    default: return 1;
  }
  shape[0] = pl.lc.threads;
  shape[1] = pl.lc.blocks;
  shape[2] = static_cast<int64_t>(pl.lc.lds);
  shape[3] = pl.resident;
  return 0;
}
