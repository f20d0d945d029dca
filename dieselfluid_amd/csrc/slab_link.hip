// slab_link.hip -- multi-GPU behind the C ABI: an RCCL communicator handle and the slab step
// drivers (the halo / migrant exchange of a slab with its two neighbours, the split WCSPH step that
// hides it under the interior force launch, the PCISPH step with its per-iteration error
// all-reduce, the periodic re-plan of the message sizes, the re-balancing of the slab planes).
// Host code only: the passes it drives and the slab primitives that launch kernels (pack, append) are
// in dslsph.hip (engine.hpp), the re-balancing count in slab_balance.hip.  gfx950 / ROCm only.
//
// RCCL is bound at run time (dlopen "librccl.so.1"), not linked: a single-GPU host never loads the
// 570 MB library, and a process that already carries an RCCL of that SONAME (PyTorch bundles one)
// gets that same copy instead of a second one with its own global state.
#include "engine.hpp"

#include <dlfcn.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "slab_balance.hpp"

using namespace dsl;

struct dsl_comm {
  ncclComm_t comm = nullptr;
  int nranks = 0, rank = 0, device = 0;
  bool custom = false;  // dsl_comm_create_custom: the host's transport table instead of RCCL
  dsl_transport tr{};
  std::string err;
};

namespace {

struct RcclApi {
  void* lib = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr;
  ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
  std::string err;
};

RcclApi& rccl() {
  static RcclApi api;
  return api;
}

bool rccl_load() {
  RcclApi& a = rccl();
  if (a.lib) return true;
  const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
  for (const char* n : names) {
    a.lib = dlopen(n, RTLD_NOW | RTLD_LOCAL);
    if (a.lib) break;
  }
  if (!a.lib) {
    a.err = std::string("cannot load RCCL: ") + (dlerror() ? dlerror() : "librccl.so.1 not found");
    return false;
  }
  bool ok = true;
  auto sym = [&](const char* s) {
    void* p = dlsym(a.lib, s);
    if (!p) {
      ok = false;
      a.err = std::string("RCCL symbol missing: ") + s;
    }
    return p;
  };
  a.GetUniqueId = reinterpret_cast<decltype(a.GetUniqueId)>(sym("ncclGetUniqueId"));
  a.CommInitRank = reinterpret_cast<decltype(a.CommInitRank)>(sym("ncclCommInitRank"));
  a.CommInitAll = reinterpret_cast<decltype(a.CommInitAll)>(sym("ncclCommInitAll"));
  a.CommDestroy = reinterpret_cast<decltype(a.CommDestroy)>(sym("ncclCommDestroy"));
  a.CommCount = reinterpret_cast<decltype(a.CommCount)>(sym("ncclCommCount"));
  a.Send = reinterpret_cast<decltype(a.Send)>(sym("ncclSend"));
  a.Recv = reinterpret_cast<decltype(a.Recv)>(sym("ncclRecv"));
  a.AllReduce = reinterpret_cast<decltype(a.AllReduce)>(sym("ncclAllReduce"));
  a.GroupStart = reinterpret_cast<decltype(a.GroupStart)>(sym("ncclGroupStart"));
  a.GroupEnd = reinterpret_cast<decltype(a.GroupEnd)>(sym("ncclGroupEnd"));
  a.GetErrorString = reinterpret_cast<decltype(a.GetErrorString)>(sym("ncclGetErrorString"));
  if (!ok) {
    dlclose(a.lib);
    a.lib = nullptr;
  }
  return ok;
}

std::string g_comm_error;

#define NCCL_TRY_H(h, expr)                                                                             \
  do {                                                                                                  \
    ncclResult_t r__ = (expr);                                                                          \
    if (r__ != ncclSuccess) return fail((h), DSL_ERR_DEVICE, std::string(#expr) + ": " + rccl().GetErrorString(r__)); \
  } while (0)

// The slab drivers' transport calls: RCCL, or the host's table (dsl_comm_create_custom) -- the SAME call
// sequence either way, which is what lets the N > 1 protocol (message order between distinct ranks, the
// re-plan and PCISPH all-reduces) run in tests on a box where RCCL cannot (several ranks on one device).
// The all-reduce words are non-negative (status counts, the bits of a non-negative float): signed and
// unsigned MAX agree on them.
#define XFER_TRY_H(h, expr, what)                                                                        \
  do {                                                                                                   \
    if ((expr) != 0) return fail((h), DSL_ERR_DEVICE, std::string("transport callback failed: ") + (what)); \
  } while (0)
inline int xfer_group_start(dsl_handle* h, dsl_comm* c) {
  if (c->custom) {
    XFER_TRY_H(h, c->tr.group_start(c->tr.ctx), "group_start");
    return DSL_OK;
  }
  NCCL_TRY_H(h, rccl().GroupStart());
  return DSL_OK;
}
inline int xfer_group_end(dsl_handle* h, dsl_comm* c) {
  if (c->custom) {
    XFER_TRY_H(h, c->tr.group_end(c->tr.ctx), "group_end");
    return DSL_OK;
  }
  NCCL_TRY_H(h, rccl().GroupEnd());
  return DSL_OK;
}
inline int xfer_send(dsl_handle* h, dsl_comm* c, const float* buf, size_t n, int peer, hipStream_t st) {
  if (c->custom) {
    XFER_TRY_H(h, c->tr.send(c->tr.ctx, buf, n * sizeof(float), peer, (void*)st), "send");
    return DSL_OK;
  }
  NCCL_TRY_H(h, rccl().Send(buf, n, ncclFloat, peer, c->comm, st));
  return DSL_OK;
}
inline int xfer_recv(dsl_handle* h, dsl_comm* c, float* buf, size_t n, int peer, hipStream_t st) {
  if (c->custom) {
    XFER_TRY_H(h, c->tr.recv(c->tr.ctx, buf, n * sizeof(float), peer, (void*)st), "recv");
    return DSL_OK;
  }
  NCCL_TRY_H(h, rccl().Recv(buf, n, ncclFloat, peer, c->comm, st));
  return DSL_OK;
}
inline int xfer_all_reduce_max(dsl_handle* h, dsl_comm* c, void* words, size_t count, hipStream_t st) {
  if (c->custom) {
    XFER_TRY_H(h, c->tr.all_reduce_max_u32(c->tr.ctx, words, count, (void*)st), "all_reduce_max_u32");
    return DSL_OK;
  }
  NCCL_TRY_H(h, rccl().AllReduce(words, words, count, ncclUint32, ncclMax, c->comm, st));
  return DSL_OK;
}

}  // namespace

// Re-balancing by moving the slab planes (dsl_slab_rebalance).  Planes are counted in cell layers from
// `origin`; planes[r] is the plane between ranks r - 1 and r, planes[0] and planes[nranks] the domain ends.
struct SlabBalance {
  int every = 0;  // steps between looks; 0 = off
  float origin = 0.f;
  int n_layers = 0, min_layers = 2, nranks = 1, rank = 0;
  // `planes`: the last plan -- in force, except for the move that `pending` says the next step still has to apply
  std::vector<int32_t> planes, plane_min, plane_max;
  std::vector<int32_t> counts;  // the last global histogram (empty before the first look)
  bool pending = false;
  int64_t looks = 0, moves = 0;
  int32_t* dev_counts = nullptr;  // kBalMaxLayers words
};

// The slab's link to its neighbours (dsl_slab_attach): communicator, neighbour ranks, message
// buffers, the side stream the transfer runs on.
struct SlabLink {
  dsl_comm* comm = nullptr;
  int lo = -1, hi = -1;  // neighbour ranks; -1 = domain end
  float width_full = 0.f, width = 0.f;
  int cap_full = 0, cap_x = 0, max_full = 0, max_x = 0;
  bool overlap = false, ghosts_in = false;
  float* send[2] = {nullptr, nullptr};
  float* recv[2] = {nullptr, nullptr};
  size_t buf_floats = 0;
  int* dev_words = nullptr;  // 4 ints for the re-plan all-reduce
  hipStream_t comm_stream = nullptr;
  hipEvent_t ev_pack = nullptr, ev_xfer = nullptr;
  int64_t steps = 0;
  int replan_every = 8;
  // periodic images along the slab axis: records arriving from the lower / upper neighbour are moved by
  // these amounts (a ring closes with -L / +L at its two end ranks; 0 elsewhere)
  float shift_from_lo = 0.f, shift_from_hi = 0.f;
  SlabBalance bal;  // dsl_slab_rebalance
};

namespace {
// The plan: a pure integer function of values every rank holds identically (slab.plan_planes is the same rule in
// Python; the tests hold the two equal).  Interior plane r aims at the k that minimises |S(k) R - r N| -- S the prefix
// sum of the counts, N their total, R the number of ranks, the smallest k on a tie -- and moves ONE layer towards it,
// unless that leaves its bounds or could leave one of the two slabs it separates thinner than min_layers: the plane
// below has already been decided, the plane above, if it is an interior one, may itself come one layer closer.
// Returns the number of planes that moved; `out` has R + 1 entries, the end planes are copied.
inline int slab_plan_planes(const int32_t* counts, int n_layers, int R, const int32_t* planes, const int32_t* plane_min,
                            const int32_t* plane_max, int min_layers, int32_t* out) {
  for (int r = 0; r <= R; ++r) out[r] = planes[r];
  long long N = 0;
  for (int k = 0; k < n_layers; ++k) N += counts[k];
  if (N == 0) return 0;
  int moved = 0;
  for (int r = 1; r < R; ++r) {
    long long S = 0, best = (long long)r * N;  // k = 0: S = 0
    int T = 0;
    for (int k = 1; k <= n_layers; ++k) {
      S += counts[k - 1];
      long long d = S * R - (long long)r * N;
      if (d < 0) d = -d;
      if (d < best) {
        best = d;
        T = k;
      }
    }
    const int q = planes[r] + (T > planes[r] ? 1 : (T < planes[r] ? -1 : 0));
    if (q == planes[r] || q < plane_min[r] || q > plane_max[r]) continue;
    const int above = planes[r + 1] - (r + 1 < R ? 1 : 0);
    if (q - out[r - 1] < min_layers || above - q < min_layers) continue;
    out[r] = q;
    ++moved;
  }
  return moved;
}
}  // namespace

// ---------------------------------------------------------------------------------------
// the communicator
// ---------------------------------------------------------------------------------------
const char* dsl_comm_last_error(void) { return g_comm_error.c_str(); }

int dsl_comm_unique_id(uint8_t id[DSL_COMM_ID_BYTES]) {
  if (!id) return DSL_ERR_INVALID;
  if (!rccl_load()) {
    g_comm_error = rccl().err;
    return DSL_ERR_UNSUPPORTED;
  }
  static_assert(DSL_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "unique id size");
  ncclUniqueId u;
  const ncclResult_t r = rccl().GetUniqueId(&u);
  if (r != ncclSuccess) {
    g_comm_error = std::string("ncclGetUniqueId: ") + rccl().GetErrorString(r);
    return DSL_ERR_DEVICE;
  }
  std::memcpy(id, u.internal, DSL_COMM_ID_BYTES);
  return DSL_OK;
}

int dsl_comm_create(int nranks, int rank, const uint8_t id[DSL_COMM_ID_BYTES], int device, dsl_comm** out) {
  if (!out || !id || nranks < 1 || rank < 0 || rank >= nranks) {
    g_comm_error = "dsl_comm_create: bad argument";
    return DSL_ERR_INVALID;
  }
  *out = nullptr;
  if (!rccl_load()) {
    g_comm_error = rccl().err;
    return DSL_ERR_UNSUPPORTED;
  }
  if (hipSetDevice(device) != hipSuccess) {
    g_comm_error = "dsl_comm_create: hipSetDevice failed";
    return DSL_ERR_DEVICE;
  }
  ncclUniqueId u;
  std::memcpy(u.internal, id, DSL_COMM_ID_BYTES);
  dsl_comm* c = new (std::nothrow) dsl_comm();
  if (!c) return DSL_ERR_NOMEM;
  const ncclResult_t r = rccl().CommInitRank(&c->comm, nranks, u, rank);
  if (r != ncclSuccess) {
    g_comm_error = std::string("ncclCommInitRank: ") + rccl().GetErrorString(r);
    delete c;
    return DSL_ERR_DEVICE;
  }
  c->nranks = nranks;
  c->rank = rank;
  c->device = device;
  *out = c;
  return DSL_OK;
}

int dsl_comm_create_all(int ndev, const int* devices, dsl_comm** out) {
  if (!out || !devices || ndev < 1) {
    g_comm_error = "dsl_comm_create_all: bad argument";
    return DSL_ERR_INVALID;
  }
  if (!rccl_load()) {
    g_comm_error = rccl().err;
    return DSL_ERR_UNSUPPORTED;
  }
  std::vector<ncclComm_t> comms((size_t)ndev);
  const ncclResult_t r = rccl().CommInitAll(comms.data(), ndev, devices);
  if (r != ncclSuccess) {
    g_comm_error = std::string("ncclCommInitAll: ") + rccl().GetErrorString(r);
    return DSL_ERR_DEVICE;
  }
  for (int k = 0; k < ndev; ++k) {
    dsl_comm* c = new dsl_comm();
    c->comm = comms[(size_t)k];
    c->nranks = ndev;
    c->rank = k;
    c->device = devices[k];
    out[k] = c;
  }
  return DSL_OK;
}

int dsl_comm_create_custom(int nranks, int rank, int device, const dsl_transport* t, dsl_comm** out) {
  if (!out || !t || nranks < 1 || rank < 0 || rank >= nranks || !t->group_start || !t->group_end || !t->send || !t->recv ||
      !t->all_reduce_max_u32) {
    g_comm_error = "dsl_comm_create_custom: bad argument (every callback of dsl_transport is required)";
    return DSL_ERR_INVALID;
  }
  dsl_comm* c = new (std::nothrow) dsl_comm();
  if (!c) return DSL_ERR_NOMEM;
  c->custom = true;
  c->tr = *t;
  c->nranks = nranks;
  c->rank = rank;
  c->device = device;
  *out = c;
  return DSL_OK;
}

int dsl_comm_destroy(dsl_comm* c) {
  if (!c) return DSL_OK;
  if (c->comm && !c->custom && rccl().lib) (void)rccl().CommDestroy(c->comm);
  delete c;
  return DSL_OK;
}

int dsl_comm_count(dsl_comm* c, int* nranks) {
  if (!c || !nranks) {
    g_comm_error = "dsl_comm_count: bad argument";
    return DSL_ERR_INVALID;
  }
  *nranks = c->nranks;
  if (!c->custom && c->comm) {
    int n = 0;
    const ncclResult_t r = rccl().CommCount(c->comm, &n);
    if (r != ncclSuccess) {
      g_comm_error = std::string("ncclCommCount: ") + rccl().GetErrorString(r);
      return DSL_ERR_DEVICE;
    }
    *nranks = n;
  }
  return DSL_OK;
}

int dsl_create_multi(const dsl_params* params, int ndev, const int* devices, dsl_handle** handles, dsl_comm** comms) {
  if (!params || !devices || !handles || !comms || ndev < 1) return fail(nullptr, DSL_ERR_INVALID, "dsl_create_multi: bad argument");
  for (int k = 0; k < ndev; ++k) handles[k] = nullptr, comms[k] = nullptr;
  for (int k = 0; k < ndev; ++k) {
    if (int rc = dsl_create(&params[k], devices[k], &handles[k])) {
      for (int j = 0; j < k; ++j) (void)dsl_destroy(handles[j]), handles[j] = nullptr;
      return rc;
    }
  }
  if (int rc = dsl_comm_create_all(ndev, devices, comms)) {
    for (int j = 0; j < ndev; ++j) (void)dsl_destroy(handles[j]), handles[j] = nullptr;
    return fail(nullptr, rc, g_comm_error);
  }
  return DSL_OK;
}

// ---------------------------------------------------------------------------------------
// the slab link and the step drivers
// ---------------------------------------------------------------------------------------
int dsl_slab_detach(dsl_handle* h) {
  if (!h || !h->link) return DSL_OK;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  SlabLink* L = h->link;
  if (L->comm_stream) (void)hipStreamSynchronize(L->comm_stream);
  for (int k = 0; k < 2; ++k) {
    (void)hipFree(L->send[k]);
    (void)hipFree(L->recv[k]);
  }
  (void)hipFree(L->dev_words);
  (void)hipFree(L->bal.dev_counts);
  if (L->ev_pack) (void)hipEventDestroy(L->ev_pack);
  if (L->ev_xfer) (void)hipEventDestroy(L->ev_xfer);
  if (L->comm_stream) (void)hipStreamDestroy(L->comm_stream);
  delete L;
  h->link = nullptr;
  return DSL_OK;
}

int dsl_slab_attach(dsl_handle* h, dsl_comm* comm, int lo_rank, int hi_rank, float width_full, float width, int cap_full,
                    int cap_xonly, int overlap) {
  CHECK_HANDLE(h);
  if (!h->c.n_ptr) return fail(h, DSL_ERR_INVALID, "dsl_slab_attach: call dsl_slab_config first");
  if ((lo_rank >= 0 || hi_rank >= 0) && !comm) return fail(h, DSL_ERR_INVALID, "dsl_slab_attach: neighbours need a communicator");
  if (comm && (lo_rank >= comm->nranks || hi_rank >= comm->nranks))
    return fail(h, DSL_ERR_INVALID, "dsl_slab_attach: neighbour rank outside the communicator");
  if (cap_full < 0 || cap_xonly < 0 || !(width_full >= 0.0f) || !(width >= width_full))
    return fail(h, DSL_ERR_INVALID, "dsl_slab_attach: bad widths or capacities");
  if (overlap && !use_tiled(h)) return fail(h, DSL_ERR_UNSUPPORTED, "dsl_slab_attach: the split step needs DSL_MATH_FAST");
  (void)dsl_slab_detach(h);
  SlabLink* L = new (std::nothrow) SlabLink();
  if (!L) return fail(h, DSL_ERR_NOMEM, "dsl_slab_attach: out of host memory");
  h->link = L;
  L->comm = comm;
  L->lo = lo_rank;
  L->hi = hi_rank;
  L->width_full = width_full;
  L->width = width;
  L->cap_full = cap_full;
  L->cap_x = cap_xonly;
  L->max_full = 2 * cap_full;  // room for the re-plan to grow the messages (the same on every rank)
  L->max_x = 2 * cap_xonly;
  L->overlap = overlap != 0 && (lo_rank >= 0 || hi_rank >= 0);
  L->buf_floats = (size_t)(L->max_full + 1) * kRecordPci + (size_t)L->max_x * kRecordX;  // (13-float records once PCISPH runs)
  for (int k = 0; k < 2; ++k) {
    if (int rc = dev_alloc(h, &L->send[k], L->buf_floats)) return rc;
    if (int rc = dev_alloc(h, &L->recv[k], L->buf_floats)) return rc;
    HIP_TRY(h, hipMemsetAsync(L->send[k], 0, L->buf_floats * sizeof(float), h->stream));
    HIP_TRY(h, hipMemsetAsync(L->recv[k], 0, L->buf_floats * sizeof(float), h->stream));
  }
  if (int rc = dev_alloc(h, &L->dev_words, 4)) return rc;
  {  // the transfer stream gets the highest priority: a hardware queue of its own (two plain streams may share
     // one, and then the transfer kernels wait behind the interior force launch they are meant to run under)
    int least = 0, greatest = 0;
    HIP_TRY(h, hipDeviceGetStreamPriorityRange(&least, &greatest));
    HIP_TRY(h, hipStreamCreateWithPriority(&L->comm_stream, hipStreamNonBlocking, greatest));
  }
  HIP_TRY(h, hipEventCreateWithFlags(&L->ev_pack, hipEventDisableTiming));
  HIP_TRY(h, hipEventCreateWithFlags(&L->ev_xfer, hipEventDisableTiming));
  if (L->overlap) {
    if (int rc = dsl_slab_split(h, width, h->split_margin > 0.0f ? h->split_margin : width)) return rc;
  }
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return DSL_OK;
}

namespace {
// one fixed-size message per neighbour and direction, all four transfers in one RCCL group
int link_post(dsl_handle* h, hipStream_t st) {
  SlabLink& L = *h->link;
  if (L.lo < 0 && L.hi < 0) return DSL_OK;
  const size_t n = dsl_slab_message_floats_for(h, L.cap_full, L.cap_x);
  dsl_comm* comm = L.comm;
  if (int rc = xfer_group_start(h, comm)) return rc;
  // (an error between group start and group end must not leave the group open: every later RCCL call of the
  // process would be queued into it and nothing would ever be sent -- close it, keep the first error)
  auto body = [&]() -> int {
    if (L.lo >= 0)
      if (int rc = xfer_send(h, comm, L.send[0], n, L.lo, st)) return rc;
    if (L.hi >= 0)
      if (int rc = xfer_send(h, comm, L.send[1], n, L.hi, st)) return rc;
    // two messages between the same pair of ranks (two ranks with periodic images, or a rank that is
    // its own neighbour in a test) are matched in issue order: the peer's LOW band arrives from above
    const bool same_peer = L.lo >= 0 && L.lo == L.hi;
    if (same_peer) {
      if (int rc = xfer_recv(h, comm, L.recv[1], n, L.hi, st)) return rc;
      if (int rc = xfer_recv(h, comm, L.recv[0], n, L.lo, st)) return rc;
    } else {
      if (L.lo >= 0)
        if (int rc = xfer_recv(h, comm, L.recv[0], n, L.lo, st)) return rc;
      if (L.hi >= 0)
        if (int rc = xfer_recv(h, comm, L.recv[1], n, L.hi, st)) return rc;
    }
    return DSL_OK;
  };
  const int rc = body();
  if (rc != DSL_OK) {
    const std::string first = h->err;
    (void)xfer_group_end(h, comm);
    h->err = first;
    return rc;
  }
  return xfer_group_end(h, comm);
}

int link_append(dsl_handle* h) {
  SlabLink& L = *h->link;
  if (L.lo < 0 && L.hi < 0) return DSL_OK;
  if (int rc = slab_append_shifted(h, L.lo >= 0 ? L.recv[0] : nullptr, L.hi >= 0 ? L.recv[1] : nullptr, L.cap_full, L.cap_x,
                                   L.shift_from_lo, L.shift_from_hi))
    return rc;
  L.ghosts_in = true;
  return DSL_OK;
}

// the band selection into the link's send buffers, one per neighbour there is
int link_pack(dsl_handle* h, hipStream_t st, float width, bool from_output) {
  SlabLink& L = *h->link;
  return slab_pack_on(h, st, L.width_full, width, from_output, L.lo >= 0 ? L.send[0] : nullptr, L.hi >= 0 ? L.send[1] : nullptr,
                      L.cap_full, L.cap_x);
}

// unsplit exchange on the handle's stream: pack, transfer, append
int link_exchange(dsl_handle* h) {
  SlabLink& L = *h->link;
  if (L.lo < 0 && L.hi < 0) return DSL_OK;
  if (int rc = link_pack(h, h->stream, L.width, false)) return rc;
  if (int rc = link_post(h, h->stream)) return rc;
  return link_append(h);
}

// ---- re-balancing: the slab planes move with the particles (dsl_slab_rebalance) ----
// where layer plane k lies: the one expression every check and every move uses
float balance_plane(const dsl_handle* h, float origin, int k) { return origin + (float)k * h->c.cell; }

// is `x` on a cell plane of the handle's grid along the slab axis (1e-3 cell of slack, as update_split allows)?
bool on_cell_plane(const dsl_handle* h, float x) {
  const float f = (x - h->c.gmin[h->c.slab_axis]) * h->c.inv_cell;
  return std::fabs(f - std::nearbyint(f)) <= 1.0e-3f;
}

// the fullest layer next to an interior plane in the last global histogram; -1 before the first look
long long balance_adjacent_max(const SlabBalance& B) {
  if (B.counts.empty()) return -1;
  long long m = 0;
  for (int r = 1; r < B.nranks; ++r)
    for (int k = B.planes[(size_t)r] - 1; k <= B.planes[(size_t)r]; ++k)
      if (k >= 0 && k < B.n_layers && B.counts[(size_t)k] > m) m = B.counts[(size_t)k];
  return m;
}

// owned particles per layer into dev_counts (overwritten), on the handle's stream
int layer_counts_on(dsl_handle* h, float origin, int n_layers, int32_t* dev_counts) {
  HIP_TRY(h, hipMemsetAsync(dev_counts, 0, sizeof(int32_t) * (size_t)n_layers, h->stream));
  launch_slab_layer_count(h->stream, h->c, launch_n(h), cpos(h), origin, n_layers, dev_counts);
  HIP_TRY(h, hipGetLastError());
  return DSL_OK;
}

// new planes on the host; the particles are not touched.  Between an integrate and the pack that follows it ownership
// is positional among the live particles (every ghost is NaN): whoever lies outside the new planes leaves as a migrant.
void move_planes(dsl_handle* h, float lo, float hi) {
  h->c.slab_lo = lo;
  h->c.slab_hi = hi;
  update_split(h);
  h->grid_valid = false;  // the owning / band / interior tile lists are made by the neighbour build
}

// The look: count, one MAX all-reduce over n_layers words (the ranks' histograms are disjoint -- one owner per live
// particle, planes on layer boundaries -- so the MAX of the non-negative counts is their sum), one host synchronisation,
// the plan.  A plan that moves a plane is applied by the NEXT step, between its integrate and its pack.
int balance_look(dsl_handle* h) {
  SlabLink& L = *h->link;
  SlabBalance& B = L.bal;
  if (int rc = layer_counts_on(h, B.origin, B.n_layers, B.dev_counts)) return rc;
  if (L.comm && L.comm->nranks > 1)
    if (int rc = xfer_all_reduce_max(h, L.comm, B.dev_counts, (size_t)B.n_layers, h->stream)) return rc;
  B.counts.resize((size_t)B.n_layers);
  HIP_TRY(h, hipMemcpyAsync(B.counts.data(), B.dev_counts, sizeof(int32_t) * (size_t)B.n_layers, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  std::vector<int32_t> next(B.planes.size());
  const int moved = slab_plan_planes(B.counts.data(), B.n_layers, B.nranks, B.planes.data(), B.plane_min.data(),
                                     B.plane_max.data(), B.min_layers, next.data());
  B.planes.swap(next);
  B.pending = B.pending || moved > 0;
  B.moves += moved;
  B.looks++;
  return DSL_OK;
}

void balance_apply(dsl_handle* h) {
  SlabBalance& B = h->link->bal;
  B.pending = false;
  // (a domain end stays where dsl_slab_config put it: -INFINITY / INFINITY, usually)
  const float lo = B.rank > 0 ? balance_plane(h, B.origin, B.planes[(size_t)B.rank]) : h->c.slab_lo;
  const float hi = B.rank + 1 < B.nranks ? balance_plane(h, B.origin, B.planes[(size_t)B.rank + 1]) : h->c.slab_hi;
  move_planes(h, lo, hi);
}

// every rank learns the largest band counts (and any overflow) seen anywhere since the last
// re-plan; all ranks switch to the same new message capacities.  Blocking.
int link_replan(dsl_handle* h) {
  SlabLink& L = *h->link;
  int32_t st[4] = {0, 0, 0, 0};
  if (int rc = dsl_slab_status(h, st, 1)) return rc;
  if (L.comm && L.comm->nranks > 1) {
    HIP_TRY(h, hipMemcpyAsync(L.dev_words, st, sizeof(st), hipMemcpyHostToDevice, h->stream));
    if (int rc = xfer_all_reduce_max(h, L.comm, L.dev_words, 4, h->stream)) return rc;  // (counts: never negative)
    HIP_TRY(h, hipMemcpyAsync(st, L.dev_words, sizeof(st), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
  }
  if (st[0] != 0)
    return fail(h, DSL_ERR_OVERFLOW,
                "slab exchange overflow: " + std::to_string(st[0]) +
                    " records did not fit a band message or the particle capacity on some rank; particles were lost -- "
                    "enlarge cap_full / cap_xonly / dsl_params.capacity");
  if (st[1] != 0)
    return fail(h, DSL_ERR_OVERFLOW, "split slab step: a particle outran the margin on some rank (ghosts were missed); enlarge the margin");
  long long want_full = (long long)(1.15 * st[2]) + 1024;
  const long long want_x = (long long)(1.15 * st[3]) + 1024;
  if (L.bal.every > 0) {
    // a plane that moves sends one cell layer of migrants on top of the h band: room for the fullest layer next to an
    // interior plane, by the last global histogram (the same numbers on every rank); before the first look there is
    // none, and the capacity the host attached with -- sized for band + layer -- is kept
    const long long layer = balance_adjacent_max(L.bal);
    want_full = layer >= 0 ? want_full + layer : (want_full > L.cap_full ? want_full : L.cap_full);
  }
  L.cap_full = (int)(want_full < L.max_full ? want_full : L.max_full);
  L.cap_x = (int)(want_x < L.max_x ? want_x : L.max_x);
  return DSL_OK;
}
}  // namespace

int dsl_slab_image_shift(dsl_handle* h, float from_lo, float from_hi) {
  CHECK_HANDLE(h);
  if (!h->link) return fail(h, DSL_ERR_INVALID, "dsl_slab_image_shift: call dsl_slab_attach first");
  h->link->shift_from_lo = from_lo;
  h->link->shift_from_hi = from_hi;
  return DSL_OK;
}

int dsl_slab_exchange(dsl_handle* h) {
  CHECK_HANDLE(h);
  if (!h->link) return fail(h, DSL_ERR_INVALID, "dsl_slab_exchange: call dsl_slab_attach first");
  if (h->split_pending) return fail(h, DSL_ERR_INVALID, "dsl_slab_exchange: a split force pass is in flight");
  return link_exchange(h);
}

int dsl_slab_replan(dsl_handle* h) {
  CHECK_HANDLE(h);
  if (!h->link) return fail(h, DSL_ERR_INVALID, "dsl_slab_replan: call dsl_slab_attach first");
  return link_replan(h);
}

int dsl_slab_layer_counts(dsl_handle* h, float origin, int n_layers, int32_t* dev_counts) {
  CHECK_HANDLE(h);
  if (!h->c.n_ptr) return fail(h, DSL_ERR_INVALID, "dsl_slab_layer_counts: no slab configured");
  if (!dev_counts) return fail(h, DSL_ERR_INVALID, "dsl_slab_layer_counts: null output");
  if (n_layers < 1 || n_layers > kBalMaxLayers)
    return fail(h, DSL_ERR_INVALID, "dsl_slab_layer_counts: n_layers must be between 1 and " + std::to_string(kBalMaxLayers));
  if (!std::isfinite(origin) || !on_cell_plane(h, origin))
    return fail(h, DSL_ERR_INVALID, "dsl_slab_layer_counts: origin is not on a cell plane of this handle's grid");
  return layer_counts_on(h, origin, n_layers, dev_counts);
}

int dsl_slab_move_planes(dsl_handle* h, float lo, float hi) {
  CHECK_HANDLE(h);
  if (!h->c.n_ptr) return fail(h, DSL_ERR_INVALID, "dsl_slab_move_planes: no slab configured");
  if (!(lo < hi)) return fail(h, DSL_ERR_INVALID, "dsl_slab_move_planes: empty range");
  if (h->split_pending) return fail(h, DSL_ERR_INVALID, "dsl_slab_move_planes: a split force pass is in flight");
  move_planes(h, lo, hi);
  return DSL_OK;
}

int dsl_slab_get_planes(dsl_handle* h, float* lo, float* hi) {
  CHECK_HANDLE_ONLY(h);
  if (!h->c.n_ptr) return fail(h, DSL_ERR_INVALID, "dsl_slab_get_planes: no slab configured");
  if (lo) *lo = h->c.slab_lo;
  if (hi) *hi = h->c.slab_hi;
  return DSL_OK;
}

int dsl_slab_rebalance(dsl_handle* h, int every, float origin, int n_layers, const int32_t* planes, const int32_t* plane_min,
                       const int32_t* plane_max, int min_layers) {
  CHECK_HANDLE(h);
  if (!h->link) return fail(h, DSL_ERR_INVALID, "dsl_slab_rebalance: call dsl_slab_attach first");
  SlabLink& L = *h->link;
  SlabBalance& B = L.bal;
  if (every < 0) return fail(h, DSL_ERR_INVALID, "dsl_slab_rebalance: every must be >= 0");
  if (every == 0) {  // off: no further look (a move the last look planned is still applied by the next step)
    B.every = 0;
    return DSL_OK;
  }
  const char* who = "dsl_slab_rebalance: ";
  if (n_layers < 1 || n_layers > kBalMaxLayers)
    return fail(h, DSL_ERR_INVALID, std::string(who) + "n_layers must be between 1 and " + std::to_string(kBalMaxLayers) +
                                        " (the count's histogram), got " + std::to_string(n_layers));
  if (min_layers < 2)
    return fail(h, DSL_ERR_INVALID, std::string(who) + "min_layers must be >= 2 (a slab thinner than the 2h band would leave "
                                                       "its neighbour's ghosts to two ranks), got " + std::to_string(min_layers));
  if (!planes || !plane_min || !plane_max) return fail(h, DSL_ERR_INVALID, std::string(who) + "null planes or bounds");
  if (!std::isfinite(origin) || !on_cell_plane(h, origin))
    return fail(h, DSL_ERR_INVALID, std::string(who) + "origin is not on a cell plane of this handle's grid");
  const int R = L.comm ? L.comm->nranks : 1, rank = L.comm ? L.comm->rank : 0;
  for (int r = 0; r <= R; ++r) {
    if (planes[r] < 0 || planes[r] > n_layers || (r > 0 && planes[r] - planes[r - 1] < min_layers))
      return fail(h, DSL_ERR_INVALID, std::string(who) + "planes must ascend inside [0, n_layers], min_layers apart (plane " +
                                          std::to_string(r) + ")");
    if (r > 0 && r < R && !(plane_min[r] <= planes[r] && planes[r] <= plane_max[r]))
      return fail(h, DSL_ERR_INVALID, std::string(who) + "plane " + std::to_string(r) + " lies outside its own bounds");
  }
  const int a = h->c.slab_axis;
  const float g0 = h->c.gmin[a], g1 = h->c.gmin[a] + (float)h->c.dims[a] * h->c.cell, slack = 1.0e-3f * h->c.cell;
  for (int side = 0; side < 2; ++side) {
    const int r = rank + side;
    const float cur = side == 0 ? h->c.slab_lo : h->c.slab_hi;
    if (r == 0 || r == R) continue;  // a domain end: never moves
    if (!(std::fabs(cur - balance_plane(h, origin, planes[r])) <= slack))
      return fail(h, DSL_ERR_INVALID, std::string(who) + "this rank's " + (side == 0 ? "lower" : "upper") + " plane (" +
                                          std::to_string(cur) + ") is not origin + planes[" + std::to_string(r) + "] * edge (" +
                                          std::to_string(balance_plane(h, origin, planes[r])) + ")");
    const float reach_lo = balance_plane(h, origin, plane_min[r]) - L.width, reach_hi = balance_plane(h, origin, plane_max[r]) + L.width;
    if (reach_lo < g0 - slack || reach_hi > g1 + slack)
      return fail(h, DSL_ERR_INVALID, std::string(who) + "plane " + std::to_string(r) + " with its band may reach [" +
                                          std::to_string(reach_lo) + ", " + std::to_string(reach_hi) + "], this handle's grid covers [" +
                                          std::to_string(g0) + ", " + std::to_string(g1) + "] along the slab axis");
  }
  if (!B.dev_counts)
    if (int rc = dev_alloc(h, &B.dev_counts, (size_t)kBalMaxLayers)) return rc;
  B.every = every;
  B.origin = origin;
  B.n_layers = n_layers;
  B.min_layers = min_layers;
  B.nranks = R;
  B.rank = rank;
  B.planes.assign(planes, planes + R + 1);
  B.plane_min.assign(plane_min, plane_min + R + 1);
  B.plane_max.assign(plane_max, plane_max + R + 1);
  B.counts.clear();
  B.pending = false;
  B.looks = B.moves = 0;
  return DSL_OK;
}

int dsl_slab_rebalance_state(dsl_handle* h, int32_t* planes, int32_t* counts, int64_t* looks, int64_t* moves) {
  CHECK_HANDLE(h);
  if (!h->link || h->link->bal.planes.empty())
    return fail(h, DSL_ERR_INVALID, "dsl_slab_rebalance_state: call dsl_slab_rebalance first");
  const SlabBalance& B = h->link->bal;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  if (planes) std::copy(B.planes.begin(), B.planes.end(), planes);
  if (counts)
    for (int k = 0; k < B.n_layers; ++k) counts[k] = B.counts.empty() ? 0 : B.counts[(size_t)k];
  if (looks) *looks = B.looks;
  if (moves) *moves = B.moves;
  return DSL_OK;
}

int dsl_slab_wcsph_step(dsl_handle* h, int nsteps) {
  CHECK_HANDLE(h);
  if (!h->link) return fail(h, DSL_ERR_INVALID, "dsl_slab_wcsph_step: call dsl_slab_attach first");
  SlabLink& L = *h->link;
  const bool alone = L.lo < 0 && L.hi < 0;
  // (Round 2 could replay the step's kernel segments as hipGraphs: measured 5 % SLOWER than launching its ~20 kernels one
  // by one -- the host needs 45 us per step for them either way, the GPU 500 us; profiles/r02_slab_graphs_on_off.txt.
  // Removed in round 4.)
  for (int s = 0; s < nsteps; ++s) {
    if (!L.ghosts_in)
      if (int rc = link_exchange(h)) return rc;  // first step: migrants + 2h ghosts from both neighbours
    L.ghosts_in = false;
    // counting sort (drops the previous step's ghosts), densities of owned + ghosts
    if (int rc = build_grid(h, false)) return rc;
    if (int rc = density_pass(h)) return rc;
    if (alone || !L.overlap || L.bal.pending) {
      // forces and integration of the owned particles (ghosts are marked for removal), band pack, transfer, append
      // (a rank without neighbours exchanges nothing)
      if (int rc = force_integrate(h)) return rc;
      if (int rc = collide_pass(h)) return rc;  // (only while a collider mesh is set) before the pack decides ownership
      // re-balancing: the planes of the last look's plan take over here, where every ghost is NaN and the pack that
      // follows hands over whoever lies outside them.  (Unsplit even with overlap: the band launch would have
      // integrated, and would pack, the layers of the old planes.)
      if (L.bal.pending) balance_apply(h);
      if (int rc = link_exchange(h)) return rc;
    } else {
      // band layers first; their pack and the RCCL transfer (side stream) run under the interior launch
      if (int rc = force_integrate(h, 1)) return rc;
      if (int rc = collide_pass(h)) return rc;  // (only while a collider mesh is set) the band layers, in the output half
      h->split_pending = true;
      if (int rc = link_pack(h, h->stream, h->split_width, true)) return rc;
      // the interior launch is queued BEHIND the pack and BEFORE the transfer is posted: the GPU goes straight from
      // the pack into it, the transfer kernels (side stream, behind the pack's event) join it
      HIP_TRY(h, hipEventRecord(L.ev_pack, h->stream));
      h->split_pending = false;
      if (int rc = force_integrate(h, 2)) return rc;
      if (int rc = collide_pass(h)) return rc;  // ... the other layers: queued before the append, under the transfer
      HIP_TRY(h, hipStreamWaitEvent(L.comm_stream, L.ev_pack, 0));
      if (int rc = link_post(h, L.comm_stream)) return rc;
      HIP_TRY(h, hipEventRecord(L.ev_xfer, L.comm_stream));
      HIP_TRY(h, hipStreamWaitEvent(h->stream, L.ev_xfer, 0));
      if (int rc = link_append(h)) return rc;
    }
    h->steps++;
    L.steps++;
    if (L.bal.every > 0 && L.steps % L.bal.every == 0)
      if (int rc = balance_look(h)) return rc;
    if (!alone && L.steps % L.replan_every == 0)
      if (int rc = link_replan(h)) return rc;
  }
  return DSL_OK;
}

int dsl_slab_pcisph_step(dsl_handle* h, int nsteps) {
  CHECK_HANDLE(h);
  if (!h->link) return fail(h, DSL_ERR_INVALID, "dsl_slab_pcisph_step: call dsl_slab_attach first");
  if (!h->pci_active) return fail(h, DSL_ERR_INVALID, "dsl_slab_pcisph_step: call dsl_pcisph_begin first");
  SlabLink& L = *h->link;
  const bool alone = L.lo < 0 && L.hi < 0;
  const bool reduce = L.comm && L.comm->nranks > 1;
  for (int s = 0; s < nsteps; ++s) {
    if (!L.ghosts_in)
      if (int rc = link_exchange(h)) return rc;
    L.ghosts_in = false;
    h->pci_split_guard = true;
    if (int rc = pci_begin_step(h)) return rc;
    for (int it = 0; it < h->prm.pci_max_iters; ++it) {
      if (int rc = pci_iterate(h)) return rc;
      // the early-out of pcisph_darwin.go:95-98 is decided by the maximum over all ranks: the error
      // word holds a non-negative float, whose bits order like an unsigned integer
      if (reduce)
        if (int rc = xfer_all_reduce_max(h, L.comm, &h->dstats->pci_cur_err_bits, 1, h->stream)) return rc;
      if (int rc = pci_check(h)) return rc;
    }
    h->pci_split_guard = false;
    if (int rc = pci_end_step(h)) return rc;  // Update; ghosts are marked for removal
    if (L.bal.pending) balance_apply(h);      // re-balancing: as in dsl_slab_wcsph_step (migrants carry their predictor state)
    if (int rc = link_exchange(h)) return rc;
    L.steps++;
    if (L.bal.every > 0 && L.steps % L.bal.every == 0)
      if (int rc = balance_look(h)) return rc;
    if (!alone && L.steps % L.replan_every == 0)
      if (int rc = link_replan(h)) return rc;
  }
  return DSL_OK;
}
