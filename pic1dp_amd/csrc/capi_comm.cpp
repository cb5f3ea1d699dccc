// capi_comm.cpp -- the charge sum over ranks: RCCL communicator (bound with dlopen, rccl_dyn.hpp), the one-hop
// exchange's set-up over IPC-mapped memory, and the helpers the hot path calls (src/pic1dp_interaction.F90:126-135).
#include <algorithm>
#include <mutex>

#include "ctx.hpp"

namespace pic1dp_host {

// the all-reduce of src/pic1dp_interaction.F90:132 on the stream
int allreduce_charge(pic1dp_ctx *c) {
  if (c->lay.nranks == 1 && !c->comm) return 0;
  if (!c->comm)
    return fail(PIC1DP_ERR_STATE, "nranks > 1 but no communicator: call pic1dp_hip_comm_init, connect the one-hop exchange (xchg_create / xchg_connect / set_allreduce), or use charge_local/charge_reduced");
  Span sp(c->tm, PIC1DP_IWT_MPIALLREDU, c->tm.timers_on);
  ncclResult_t r = rccl().AllReduce(c->d_charge, c->d_charge, static_cast<size_t>(c->in.nx), ncclDouble,
                                    ncclSum, c->comm, c->st);
  if (r != ncclSuccess) return fail(PIC1DP_ERR_COMM, "ncclAllReduce: %s", rccl().GetErrorString(r));
  return sp.end();
}

constexpr size_t kXchgFlagBytes = 4096;  // flags[2][XCHG_MAX_RANKS] u64, padded

// Exchange areas created in THIS process, by their IPC handle: a host that drives several ranks from one process (one
// thread per GPU, or several contexts on one GPU) hands xchg_connect handles of its own making -- hipIpcOpenMemHandle
// refuses those, and there is nothing to open: the area is addressable as it is (on another device of the process once
// peer access is enabled).
struct LocalArea {
  unsigned char handle[PIC1DP_XCHG_HANDLE_BYTES];
  void *ptr;
  int device;
};
std::mutex g_areas_mu;
std::vector<LocalArea> g_areas;

void area_register(const unsigned char *handle, void *ptr, int device) {
  std::lock_guard<std::mutex> lk(g_areas_mu);
  LocalArea a{};
  std::memcpy(a.handle, handle, sizeof a.handle);
  a.ptr = ptr;
  a.device = device;
  g_areas.push_back(a);
}
void area_forget(void *ptr) {
  std::lock_guard<std::mutex> lk(g_areas_mu);
  for (size_t i = 0; i < g_areas.size(); ++i)
    if (g_areas[i].ptr == ptr) {
      g_areas.erase(g_areas.begin() + static_cast<std::ptrdiff_t>(i));
      return;
    }
}
bool area_lookup(const unsigned char *handle, void **ptr, int *device) {
  std::lock_guard<std::mutex> lk(g_areas_mu);
  for (const LocalArea &a : g_areas)
    if (std::memcmp(a.handle, handle, sizeof a.handle) == 0) {
      *ptr = a.ptr;
      *device = a.device;
      return true;
    }
  return false;
}

bool xchg_active(const pic1dp_ctx *c) { return c->allreduce_kind == 2 && c->xc.connected; }

// a slot carries the charge and the prediction's slices (XCHG_MAX_VEC), or kind 1's integer packet (2 nspecies)
int xchg_vec(const pic1dp_ctx *c) { return std::max(XCHG_MAX_VEC, 2 * c->in.nspecies); }

XchgArgs next_xchg_args(pic1dp_ctx *c) {
  XchgArgs x{};
  for (int q = 0; q < c->lay.nranks; ++q) {
    char *b = reinterpret_cast<char *>(c->xc.peer[q]);
    x.flags[q] = reinterpret_cast<unsigned long long *>(b);
    x.slots[q] = reinterpret_cast<double *>(b + kXchgFlagBytes);
  }
  x.err = c->xc.err;
  x.epoch = ++c->xc.epoch;
  x.timeout_ticks = c->xc.timeout_ticks;
  x.rank = c->lay.rank;
  x.nranks = c->lay.nranks;
  x.vstride = xchg_vec(c) * c->in.nx;
  x.ticks = c->tm.timers_on ? c->xc.ticks : nullptr;
  return x;
}

// a time-out reported by an exchange kernel (checked wherever the host synchronises)
int xchg_check(pic1dp_ctx *c) {
  if (int rc = fx_check(c)) return rc;  // (kind 1's overflow counter: read at the same synchronisation points)
  if (!c->xc.err) return 0;
  const unsigned long long e = *reinterpret_cast<volatile unsigned long long *>(c->xc.err);
  if (e == 0) return 0;
  return fail(PIC1DP_ERR_COMM, "charge exchange %llu: rank %d waited in vain for the charge of rank %d (peer stopped or out of step)",
              e >> 8, c->lay.rank, static_cast<int>(e & 0xff) - 1);
}

// charge2 -> charge1 over ranks, whichever way is configured: the exchange kernel, or
// k_charge_local + RCCL all-reduce (src/pic1dp_interaction.F90:126-135)
int reduce_charge(pic1dp_ctx *c) {
  if (xchg_active(c)) {
    Span sp(c->tm, PIC1DP_IWT_MPIALLREDU, c->tm.timers_on);
    HIP_TRY(launch_charge_exchange(c->fa, next_xchg_args(c), c->st));
    return sp.end();
  }
  HIP_TRY(launch_charge_local(c->fa, c->st));
  return allreduce_charge(c);
}

int allreduce_doubles(pic1dp_ctx *c, double *d, size_t n) {
  if (!c->comm) {
    if (c->lay.nranks > 1)
      return fail(PIC1DP_ERR_STATE, "nranks > 1 but no communicator: reduce the local sums on the host instead");
    return 0;
  }
  ncclResult_t r = rccl().AllReduce(d, d, n, ncclDouble, ncclSum, c->comm, c->st);
  if (r != ncclSuccess) return fail(PIC1DP_ERR_COMM, "ncclAllReduce: %s", rccl().GetErrorString(r));
  return 0;
}


void comm_release(pic1dp_ctx *c) {
  if (c->comm) {
    rccl().CommDestroy(c->comm);
    c->comm = nullptr;
  }
  for (int q = 0; q < XCHG_MAX_RANKS; ++q)
    if (c->xc.opened[q]) (void)hipIpcCloseMemHandle(c->xc.peer[q]);
  if (c->xc.local) {
    area_forget(c->xc.local);
    (void)hipFree(c->xc.local);
  }
  if (c->xc.err) (void)hipHostFree(c->xc.err);
  (void)hipFree(c->xc.ticks);
}

}  // namespace pic1dp_host

extern "C" {

// ---------------------------------------------------------------------------
// RCCL
// ---------------------------------------------------------------------------
int pic1dp_hip_comm_unique_id(unsigned char id[PIC1DP_COMM_ID_BYTES]) {
  static_assert(sizeof(ncclUniqueId) == PIC1DP_COMM_ID_BYTES, "unique id size");
  if (!id) return fail(PIC1DP_ERR_ARG, "null id");
  std::string err;
  if (!rccl().load(err)) return fail(PIC1DP_ERR_COMM, "%s", err.c_str());
  ncclUniqueId u;
  ncclResult_t r = rccl().GetUniqueId(&u);
  if (r != ncclSuccess) return fail(PIC1DP_ERR_COMM, "ncclGetUniqueId: %s", rccl().GetErrorString(r));
  std::memcpy(id, u.internal, PIC1DP_COMM_ID_BYTES);
  return 0;
}

int pic1dp_hip_comm_init(pic1dp_ctx *c, const unsigned char id[PIC1DP_COMM_ID_BYTES]) {
  CHECK_CTX(c);
  if (!id) return fail(PIC1DP_ERR_ARG, "null id");
  if (c->comm) return fail(PIC1DP_ERR_STATE, "communicator already initialised");
  std::string err;
  if (!rccl().load(err)) return fail(PIC1DP_ERR_COMM, "%s", err.c_str());
  HIP_TRY(hipSetDevice(c->device));
  ncclUniqueId u;
  std::memcpy(u.internal, id, PIC1DP_COMM_ID_BYTES);
  ncclResult_t r = rccl().CommInitRank(&c->comm, c->lay.nranks, u, c->lay.rank);
  if (r != ncclSuccess) {
    c->comm = nullptr;
    return fail(PIC1DP_ERR_COMM, "ncclCommInitRank: %s", rccl().GetErrorString(r));
  }
  return 0;
}

// ---------------------------------------------------------------------------
// one-hop charge exchange over peer-mapped memory (alternative to the RCCL
// all-reduce; kernels_field.hip exchange_charge)
// ---------------------------------------------------------------------------
int pic1dp_hip_comm_available(void) {
  std::string err;
  if (!rccl().load(err)) return fail(PIC1DP_ERR_COMM, "%s", err.c_str());
  return 0;
}

int pic1dp_hip_xchg_create(pic1dp_ctx *c, unsigned char handle[PIC1DP_XCHG_HANDLE_BYTES]) {
  static_assert(sizeof(hipIpcMemHandle_t) == PIC1DP_XCHG_HANDLE_BYTES, "ipc handle size");
  CHECK_CTX(c);
  if (!handle) return fail(PIC1DP_ERR_ARG, "null handle");
  if (c->lay.nranks > XCHG_MAX_RANKS) return fail(PIC1DP_ERR_ARG, "the exchange serves at most %d ranks", XCHG_MAX_RANKS);
  if (c->xc.local) return fail(PIC1DP_ERR_STATE, "exchange area already created");
  HIP_TRY(hipSetDevice(c->device));
  const size_t bytes = kXchgFlagBytes + sizeof(double) * 2 * static_cast<size_t>(c->lay.nranks) * xchg_vec(c) * c->in.nx;
  // memory the peers' stores and this GPU's polls meet in has to be coherent across agents INSIDE a kernel:
  // fine-grained, else uncached.  Plain (coarse-grained) hipMalloc memory is not -- a stale L2 line of the
  // same-parity slot of exchange e - 2 would be summed without any error showing -- so the automatic chain stops
  // after the two coherent kinds and reports PIC1DP_ERR_COMM (the host then agrees on RCCL or its own sum);
  // kind 3 only when PIC1DP_XCHG_MEM=3 asks for it by name (experiments).
  int want = 1, last = 2;
  if (const char *e = std::getenv("PIC1DP_XCHG_MEM")) {
    want = std::atoi(e);
    if (want < 1 || want > 3) return fail(PIC1DP_ERR_ARG, "PIC1DP_XCHG_MEM must be 1 (fine-grained), 2 (uncached) or 3 (plain)");
    last = want == 3 ? 3 : 2;
  }
  hipError_t e = hipErrorUnknown;
  for (int kind = want; kind <= last && e != hipSuccess; ++kind) {
    if (kind == 1) e = hipExtMallocWithFlags(&c->xc.local, bytes, hipDeviceMallocFinegrained);
    if (kind == 2) e = hipExtMallocWithFlags(&c->xc.local, bytes, hipDeviceMallocUncached);
    if (kind == 3) e = hipMalloc(&c->xc.local, bytes);
    hipIpcMemHandle_t h;
    if (e == hipSuccess) {
      e = hipIpcGetMemHandle(&h, c->xc.local);
      if (e == hipSuccess) {
        std::memcpy(handle, &h, sizeof h);
        c->xc.memkind = kind;
      } else {
        (void)hipFree(c->xc.local);
        c->xc.local = nullptr;
      }
    }
    if (e != hipSuccess) (void)hipGetLastError();
  }
  if (e != hipSuccess)
    return fail(PIC1DP_ERR_COMM, "exchange area: no fine-grained or uncached device memory with an IPC handle (%s)",
                hipGetErrorString(e));
  HIP_TRY(hipMemset(c->xc.local, 0, bytes));
  if (!c->xc.err) {
    HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&c->xc.err), 64, hipHostMallocDefault));
    *c->xc.err = 0;
  }
  double tmo_ms = 20000.0;
  if (const char *t = std::getenv("PIC1DP_XCHG_TIMEOUT_MS")) tmo_ms = std::atof(t);
  c->xc.timeout_ticks = static_cast<long long>(tmo_ms * 1e5);  // wall_clock64 counts at 100 MHz
  c->xc.epoch = 0;
  if (!c->xc.ticks) {
    HIP_TRY(hipMalloc(&c->xc.ticks, 2 * sizeof(unsigned long long)));
    HIP_TRY(hipMemset(c->xc.ticks, 0, 2 * sizeof(unsigned long long)));
  }
  HIP_TRY(hipDeviceSynchronize());
  area_register(handle, c->xc.local, c->device);
  return 0;
}

int pic1dp_hip_xchg_connect(pic1dp_ctx *c, const unsigned char *handles) {
  CHECK_CTX(c);
  if (!handles) return fail(PIC1DP_ERR_ARG, "null handles");
  if (!c->xc.local) return fail(PIC1DP_ERR_STATE, "xchg_connect before xchg_create");
  if (c->xc.connected) return fail(PIC1DP_ERR_STATE, "exchange already connected");
  HIP_TRY(hipSetDevice(c->device));
  for (int q = 0; q < c->lay.nranks; ++q) {
    if (q == c->lay.rank) {
      c->xc.peer[q] = c->xc.local;
      continue;
    }
    void *mine = nullptr;
    int dev = -1;
    if (area_lookup(handles + static_cast<size_t>(q) * PIC1DP_XCHG_HANDLE_BYTES, &mine, &dev)) {  // a rank of this very process
      if (dev != c->device) {
        hipError_t pe = hipDeviceEnablePeerAccess(dev, 0);
        if (pe != hipSuccess && pe != hipErrorPeerAccessAlreadyEnabled) {
          (void)hipGetLastError();
          return fail(PIC1DP_ERR_COMM, "peer access from device %d to device %d (rank %d of this process): %s", c->device, dev, q,
                      hipGetErrorString(pe));
        }
        (void)hipGetLastError();
      }
      c->xc.peer[q] = mine;
      continue;
    }
    hipIpcMemHandle_t h;
    std::memcpy(&h, handles + static_cast<size_t>(q) * PIC1DP_XCHG_HANDLE_BYTES, sizeof h);
    hipError_t e = hipIpcOpenMemHandle(&c->xc.peer[q], h, hipIpcMemLazyEnablePeerAccess);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return fail(PIC1DP_ERR_COMM, "hipIpcOpenMemHandle for the exchange area of rank %d: %s", q, hipGetErrorString(e));
    }
    c->xc.opened[q] = true;
  }
  c->xc.connected = true;
  return 0;
}

int pic1dp_hip_set_allreduce(pic1dp_ctx *c, int32_t kind) {
  CHECK_CTX(c);
  if (kind < 0 || kind > 2) return fail(PIC1DP_ERR_ARG, "allreduce kind must be 0 (auto), 1 (RCCL) or 2 (one-hop exchange)");
  if (kind == 2 && !c->xc.connected) return fail(PIC1DP_ERR_STATE, "the one-hop exchange is not connected");
  if (kind == 1 && !c->comm) return fail(PIC1DP_ERR_STATE, "no RCCL communicator");
  c->allreduce_kind = kind;
  return 0;
}

int pic1dp_hip_xchg_time(pic1dp_ctx *c, double *ms, int64_t *exchanges_timed, int32_t reset) {
  CHECK_CTX(c);
  if (ms) *ms = 0.0;
  if (exchanges_timed) *exchanges_timed = 0;
  if (!c->xc.ticks) return 0;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->st));
  unsigned long long t[2] = {0, 0};
  HIP_TRY(hipMemcpy(t, c->xc.ticks, sizeof t, hipMemcpyDeviceToHost));
  if (ms) *ms = static_cast<double>(t[0]) * 1e-5;  // 100 MHz wall clock
  if (exchanges_timed) *exchanges_timed = static_cast<int64_t>(t[1]);
  if (reset) {  // on the stream the exchange kernels run on: ordered against the next exchange's additions
    HIP_TRY(hipMemsetAsync(c->xc.ticks, 0, sizeof t, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
  }
  return xchg_check(c);
}

int pic1dp_hip_xchg_info(pic1dp_ctx *c, int32_t *memkind, int64_t *exchanges) {
  CHECK_CTX(c);
  if (memkind) *memkind = c->xc.memkind;
  if (exchanges) *exchanges = static_cast<int64_t>(c->xc.epoch);
  return xchg_check(c);
}


}  // extern "C"
