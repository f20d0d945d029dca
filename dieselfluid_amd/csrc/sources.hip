// sources.hip -- sources and sinks: fluid particles created and removed on the device (dsl_particles_append, dsl_emitter_add,
// dsl_emit, dsl_sink_add, dsl_particles_remove, and the step drivers' hook sources_step).  A translation unit of its own, so
// that every other unit's kernels come out as they are; its kernel list is tests/golden/device_kernels_sources.txt.  Same
// flags as every unit: -ffp-contract=off keeps every operation at one rounding.  The rule is build-defined
// (include/dslsph.h) and restated operation for operation in tests/sources_ref.py; it is the same in both
// math modes.
//
//   k_sources_emit   one lane per new particle: an emitter's lane k reads point k of the list the host built and makes
//                    (origin + a u) + b v; an explicit append's lane k reads the staged host arrays.  Both write every array
//                    of slot base + k: position, velocity, id, force_reset where forces are materialised, pressure 0
//                    where pressures are, density 0 and P/rho^2 0, the predictor state while PCISPH is active
//   k_sink_count     grid-stride over the slots, 12 bytes read per slot, the sinks by value: one ballot and popcount per
//                    wave and trip, one int atomic per wave that found something -- int sums, so the count is exact
//   k_sink_flag      the same test per slot, written to the particle's HOST INDEX: keep[id] (the renumbering is a prefix
//                    sum in host order, whatever order the slots are in)
//   k_sink_blocks    one count per workgroup of 256 host indices
//   k_sink_scan      one workgroup: the counts into offsets, the total behind them
//   k_sink_index     a survivor's new host index: its workgroup's offset plus its rank among the workgroup's lanes --
//                    counts and a scan, no atomic decides a position, so two runs give the same bytes
//   k_sink_gather    one lane per slot: every array's value moves to slot = new host index of the other ping-pong half
//
// After a removal the slots are in host order (ids[s] = s); the next neighbour build sorts them as it sorts any state.
#include "engine.hpp"
#include "sph_device.hpp"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

namespace dsl {

constexpr int kSrcBlock = 256;
constexpr int kSrcMaxGrid = 2048;  // workgroups of the sink count's grid-stride sweep
constexpr int kGatherFields = 18;  // pos + vel (6), forces (3), predictor state (6), rho, pterm, press

// the sinks of a handle, by value in the kernel arguments
struct SinkSet {
  int n;
  float lo[DSL_MAX_SINKS][3], hi[DSL_MAX_SINKS][3];
  int outside[DSL_MAX_SINKS];
};
// an emitter's face, by value
struct EmitFace {
  float o[3], u[3], v[3], vel[3];
  int nu;
};
// the arrays a new particle is written to (nullptr: not materialised / not active)
struct EmitOut {
  float* pv[6];
  float* frc[3];
  float* pci[6];
  float *rho, *pterm, *press;
  int* ids;
  float reset[3];
};
// the compaction's moves: src[k][slot] -> dst[k][new index]; nullptr: no such array at the moment
struct GatherArrays {
  const float* src[kGatherFields];
  float* dst[kGatherFields];
};

namespace {
// does a particle at (x, y, z) go?  inside = (x_a >= min_a && x_a < max_a) on all three axes -- false for a NaN -- and it
// goes when, for some sink, inside != (outside != 0)
__device__ __forceinline__ bool sink_takes(const SinkSet& s, float x, float y, float z) {
  bool goes = false;
#pragma unroll
  for (int k = 0; k < DSL_MAX_SINKS; ++k) {
    if (k < s.n) {  // (uniform)
      const bool inside = x >= s.lo[k][0] && x < s.hi[k][0] && y >= s.lo[k][1] && y < s.hi[k][1] && z >= s.lo[k][2] && z < s.hi[k][2];
      goes = goes || (inside != (s.outside[k] != 0));
    }
  }
  return goes;
}
}  // namespace

__global__ __launch_bounds__(kSrcBlock) void k_sources_emit(int m, int base, const int* __restrict__ pts, EmitFace f,
                                                            const float* __restrict__ xyz, const float* __restrict__ vxyz,
                                                            EmitOut o) {
  const int k = blockIdx.x * kSrcBlock + threadIdx.x;
  if (k >= m) return;
  float x[3], v[3];
  if (pts) {  // (uniform) lattice point (a, b): every product and sum rounded once
    const int w = pts[k];
    const float a = (float)(w % f.nu), b = (float)(w / f.nu);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      x[c] = __fadd_rn(__fadd_rn(f.o[c], __fmul_rn(a, f.u[c])), __fmul_rn(b, f.v[c]));
      v[c] = f.vel[c];
    }
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      x[c] = xyz[3 * (size_t)k + c];
      v[c] = vxyz ? vxyz[3 * (size_t)k + c] : 0.0f;
    }
  }
  const int s = base + k;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    o.pv[c][s] = x[c];
    o.pv[3 + c][s] = v[c];
    if (o.frc[c]) o.frc[c][s] = o.reset[c];
    if (o.pci[c]) {
      o.pci[c][s] = x[c];
      o.pci[3 + c][s] = v[c];
    }
  }
  o.rho[s] = 0.0f;
  o.pterm[s] = 0.0f;
  if (o.press) o.press[s] = 0.0f;
  o.ids[s] = s;  // (no boundary particles, no slab: the slots behind the live ones are the next host indices)
}

__global__ __launch_bounds__(kSrcBlock) void k_sink_count(int n, CSoa3 p, SinkSet sinks, int* __restrict__ count) {
  int found = 0;
  for (int base = blockIdx.x * kSrcBlock; base < n; base += gridDim.x * kSrcBlock) {  // (uniform trips)
    const int s = base + threadIdx.x;
    const bool goes = s < n && sink_takes(sinks, p.x[s], p.y[s], p.z[s]);
    found += __popcll(__ballot(goes));
  }
  if ((threadIdx.x & (kWave - 1)) == 0 && found != 0) atomicAdd(count, found);
}

// keep[host index] = 1 for a survivor; keep_first: every particle would go, host index 0 stays
__global__ __launch_bounds__(kSrcBlock) void k_sink_flag(int n, CSoa3 p, const int* __restrict__ ids, SinkSet sinks, int keep_first,
                                                         int* __restrict__ keep) {
  const int s = blockIdx.x * kSrcBlock + threadIdx.x;
  if (s >= n) return;
  const int id = ids[s];
  if (id < 0 || id >= n) return;  // (cannot happen: the ids are a permutation of 0 .. n - 1 here)
  keep[id] = (!sink_takes(sinks, p.x[s], p.y[s], p.z[s]) || (keep_first && id == 0)) ? 1 : 0;
}

namespace {
// this lane's rank among the workgroup's lanes with `on`, and the workgroup's count of them (s_wave: one int per wave)
__device__ __forceinline__ int block_rank(bool on, int* s_wave, int* total) {
  const unsigned long long bal = __ballot(on);
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  if (lane == 0) s_wave[wave] = __popcll(bal);
  lds_barrier();
  int at = 0, all = 0;
#pragma unroll
  for (int w = 0; w < kSrcBlock / kWave; ++w) {
    const int c = s_wave[w];
    if (w < wave) at += c;
    all += c;
  }
  *total = all;
  return at + __popcll(bal & ((1ull << lane) - 1ull));
}
}  // namespace

__global__ __launch_bounds__(kSrcBlock) void k_sink_blocks(int n, const int* __restrict__ keep, int* __restrict__ counts) {
  __shared__ int s_wave[kSrcBlock / kWave];
  const int i = blockIdx.x * kSrcBlock + threadIdx.x;
  int total = 0;
  (void)block_rank(i < n && keep[i] != 0, s_wave, &total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// counts[0 .. nblk) -> their exclusive prefix, counts[nblk] = the total.  One workgroup: lane t sums its run of
// ceil(nblk / 256) counts, the 256 sums are scanned in LDS, and the lane writes its run's offsets
__global__ __launch_bounds__(kSrcBlock) void k_sink_scan(int nblk, int* counts) {
  __shared__ int s[kSrcBlock];
  const int tid = threadIdx.x;
  const int run = (nblk + kSrcBlock - 1) / kSrcBlock;
  const int first = tid * run, last = min(first + run, nblk);
  int sum = 0;
  for (int i = first; i < last; ++i) sum += counts[i];
  s[tid] = sum;
  lds_barrier();
  for (int off = 1; off < kSrcBlock; off <<= 1) {
    const int t = tid >= off ? s[tid - off] : 0;
    lds_barrier();
    s[tid] += t;
    lds_barrier();
  }
  int at = s[tid] - sum;
  const int all = s[kSrcBlock - 1];
  for (int i = first; i < last; ++i) {
    const int c = counts[i];
    counts[i] = at;
    at += c;
  }
  if (tid == 0) counts[nblk] = all;
}

// index[host index] = the survivor's new host index, -1 for a particle that goes
__global__ __launch_bounds__(kSrcBlock) void k_sink_index(int n, const int* __restrict__ keep, const int* __restrict__ offsets,
                                                          int* __restrict__ index) {
  __shared__ int s_wave[kSrcBlock / kWave];
  const int i = blockIdx.x * kSrcBlock + threadIdx.x;
  const bool on = i < n && keep[i] != 0;
  int total = 0;
  const int at = offsets[blockIdx.x] + block_rank(on, s_wave, &total);
  if (i < n) index[i] = on ? at : -1;
}

__global__ __launch_bounds__(kSrcBlock) void k_sink_gather(int n, int n_after, const int* __restrict__ ids, const int* __restrict__ index,
                                                           GatherArrays a, int* __restrict__ ids_dst) {
  const int s = blockIdx.x * kSrcBlock + threadIdx.x;
  if (s >= n) return;
  const int id = ids[s];
  if (id < 0 || id >= n) return;
  const int r = index[id];
  if (r < 0 || r >= n_after) return;  // (r >= n_after cannot happen: the scan's total is n_after)
#pragma unroll
  for (int k = 0; k < kGatherFields; ++k)
    if (a.src[k]) a.dst[k][r] = a.src[k][s];  // (uniform)
  ids_dst[r] = r;
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
namespace {
inline int src_blocks(int n) { return (n + kSrcBlock - 1) / kSrcBlock; }

// what every call that changes the count, or prepares to, refuses: dsl_last_error names what to remove first
int sources_refuse(dsl_handle* h, const std::string& w) {
  if (h->c.slab_axis >= 0 || h->c.n_ptr)
    return fail(h, DSL_ERR_UNSUPPORTED, w + ": sources and sinks are not supported in slab mode (leave it with dsl_slab_config(axis = -1) first)");
  if (h->lsh) return fail(h, DSL_ERR_UNSUPPORTED, w + ": not supported with DSL_NEIGH_LSH_REF (create the handle with DSL_NEIGH_GRID)");
  if (h->nb > 0)
    return fail(h, DSL_ERR_UNSUPPORTED, w + ": not supported on a handle with boundary particles (fluid has to stay in front of them)");
  if (h->ids_global) return fail(h, DSL_ERR_UNSUPPORTED, w + ": host order is gone after dsl_set_ids");
  return DSL_OK;
}

void set_count(dsl_handle* h, int n) {
  h->n = n;
  h->c.n = n;
  h->prm.n_particles = n;
  h->count_changed = true;
  h->grid_valid = false;
  h->masks_valid = false;
  h->pci_rows_live = false;
}

EmitOut emit_out(dsl_handle* h) {
  EmitOut o{};
  for (int k = 0; k < 6; ++k) o.pv[k] = h->pv[h->cur_pv][k];
  for (int k = 0; k < 3; ++k) o.frc[k] = h->forces_uniform ? nullptr : h->frc[h->cur_f][k];
  for (int k = 0; k < 6; ++k) o.pci[k] = h->pci_active ? h->pci[h->cur_pci][k] : nullptr;
  o.rho = h->rho;
  o.pterm = h->pterm;
  o.press = h->press_zero ? nullptr : h->press;
  o.ids = h->ids[h->cur_ids];
  for (int k = 0; k < 3; ++k) o.reset[k] = h->c.reset[k];
  return o;
}

// m new particles behind the live ones: the shared launch of the explicit append (pts == nullptr) and of an emitter.
// The caller has checked that they fit
int emit_launch(dsl_handle* h, int m, const int* pts, const EmitFace& f, const float* xyz, const float* vxyz) {
  if ((long long)h->n + m > h->cap) return fail(h, DSL_ERR_NOMEM, "sources: the new particles do not fit dsl_params.capacity");
  const int rc = timed(h, DSL_K_SOURCES, [&] {
    hipLaunchKernelGGL(k_sources_emit, dim3((unsigned)src_blocks(m)), dim3(kSrcBlock), 0, h->stream, m, h->n, pts, f, xyz, vxyz,
                       emit_out(h));
  });
  if (rc) return rc;
  set_count(h, h->n + m);
  h->dens_fresh = false;  // (dens_held stays: the new slots hold density 0)
  return DSL_OK;
}

int emit_layer(dsl_handle* h, int e) {
  const dsl_emitter& d = h->emitters[e];
  EmitFace f{};
  for (int c = 0; c < 3; ++c) f.o[c] = d.origin[c], f.u[c] = d.u[c], f.v[c] = d.v[c], f.vel[c] = d.velocity[c];
  f.nu = d.nu;
  if (int rc = emit_launch(h, h->emit_m[e], h->emit_pts[e].p, f, nullptr, nullptr)) return rc;
  h->emit_layers[e] += 1;
  h->src_emitted += h->emit_m[e];
  return DSL_OK;
}

SinkSet sink_set(const dsl_handle* h) {
  SinkSet s{};
  s.n = h->n_sinks;
  for (int k = 0; k < h->n_sinks; ++k) {
    for (int a = 0; a < 3; ++a) s.lo[k][a] = h->sinks[k].box_min[a], s.hi[k][a] = h->sinks[k].box_max[a];
    s.outside[k] = h->sinks[k].outside;
  }
  return s;
}

// One look: the count kernel and its 4-byte read-back; the compaction only when the count is not 0.  Blocking.
int sinks_apply(dsl_handle* h, int64_t* removed) {
  if (removed) *removed = 0;
  if (h->n_sinks == 0) return DSL_OK;
  const int n = h->n;
  const SinkSet sinks = sink_set(h);
  if (int rc = reserve(h, h->src_ctr, 2, "sinks: the count's word")) return rc;
  HIP_TRY(h, hipMemsetAsync(h->src_ctr.p, 0, sizeof(int), h->stream));
  int rc = timed(h, DSL_K_SOURCES, [&] {
    hipLaunchKernelGGL(k_sink_count, dim3((unsigned)std::min(src_blocks(n), kSrcMaxGrid)), dim3(kSrcBlock), 0, h->stream, n, cpos(h),
                       sinks, h->src_ctr.p);
  });
  if (rc) return rc;
  int gone = 0;
  HIP_TRY(h, hipMemcpyAsync(&gone, h->src_ctr.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  if (gone <= 0) return DSL_OK;
  const int keep_first = gone >= n ? 1 : 0;  // never an empty handle: host index 0 stays
  const int n_after = keep_first ? 1 : n - gone;
  const int nblk = src_blocks(n);
  if (int rc2 = reserve(h, h->src_scan, (size_t)src_blocks(h->cap) + 1, "sinks: the compaction's counts")) return rc2;
  // (the neighbour build's scratch, free between builds: rank holds keep[], sort_keys the new indices)
  int *keep = h->rank, *index = h->sort_keys, *counts = h->src_scan.p;
  const int X = h->cur_pv, Y = X ^ 1;
  GatherArrays a{};
  int nf = 0;
  for (int k = 0; k < 6; ++k) a.src[nf] = h->pv[X][k], a.dst[nf++] = h->pv[Y][k];
  if (!h->forces_uniform)
    for (int k = 0; k < 3; ++k) a.src[nf] = h->frc[h->cur_f][k], a.dst[nf++] = h->frc[h->cur_f ^ 1][k];
  if (h->pci_active)
    for (int k = 0; k < 6; ++k) a.src[nf] = h->pci[h->cur_pci][k], a.dst[nf++] = h->pci[h->cur_pci ^ 1][k];
  // the scalars go through the three thirds of the staging array and back
  float* scalars[3] = {h->rho, h->pterm, h->press_zero ? nullptr : h->press};
  for (int k = 0; k < 3; ++k)
    if (scalars[k]) a.src[nf] = scalars[k], a.dst[nf++] = h->stage + (size_t)k * h->cap;
  const dim3 g((unsigned)nblk), b(kSrcBlock);
  const int* ids = h->ids[h->cur_ids];
  int* ids_dst = h->ids[h->cur_ids ^ 1];
  auto step = [&](auto&& launch) { return timed(h, DSL_K_SOURCES, launch); };
  if ((rc = step([&] { hipLaunchKernelGGL(k_sink_flag, g, b, 0, h->stream, n, cpos(h), ids, sinks, keep_first, keep); }))) return rc;
  if ((rc = step([&] { hipLaunchKernelGGL(k_sink_blocks, g, b, 0, h->stream, n, (const int*)keep, counts); }))) return rc;
  if ((rc = step([&] { hipLaunchKernelGGL(k_sink_scan, dim3(1), b, 0, h->stream, nblk, counts); }))) return rc;
  if ((rc = step([&] { hipLaunchKernelGGL(k_sink_index, g, b, 0, h->stream, n, (const int*)keep, (const int*)counts, index); }))) return rc;
  if ((rc = step([&] { hipLaunchKernelGGL(k_sink_gather, g, b, 0, h->stream, n, n_after, ids, (const int*)index, a, ids_dst); }))) return rc;
  for (int k = 0; k < 3; ++k)
    if (scalars[k])
      HIP_TRY(h, hipMemcpyAsync(scalars[k], h->stage + (size_t)k * h->cap, sizeof(float) * (size_t)n_after, hipMemcpyDeviceToDevice,
                                h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  h->cur_pv ^= 1;
  h->cur_ids ^= 1;
  if (!h->forces_uniform) h->cur_f ^= 1;
  if (h->pci_active) h->cur_pci ^= 1;
  set_count(h, n_after);  // (dens_held and dens_fresh stay: the survivors' densities still belong to them)
  h->src_removed += n - n_after;
  if (removed) *removed = n - n_after;
  return DSL_OK;
}

// is emitter e due at step s?
bool emitter_due(const dsl_handle* h, int e, int64_t s) {
  const dsl_emitter& d = h->emitters[e];
  return s >= d.first_step && (s - d.first_step) % d.period == 0 && (d.max_layers == 0 || h->emit_layers[e] < d.max_layers);
}
}  // namespace

void sources_free(dsl_handle* h) {
  for (auto& a : h->emit_pts) release(a);
  release(h->src_ctr);
  release(h->src_scan);
}

int sources_step(dsl_handle* h) {
  if (h->n_emitters == 0 && h->n_sinks == 0) return DSL_OK;
  const int64_t s = h->steps;
  const bool look = h->n_sinks > 0 && h->sink_every > 0 && s % h->sink_every == 0;
  bool emit = false;
  for (int e = 0; e < h->n_emitters; ++e) emit = emit || emitter_due(h, e, s);
  if (!look && !emit) return DSL_OK;
  // (a host that is capturing this stream into a graph of its own: a replayed graph cannot change its grids or wait for
  // a read-back)
  hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(h->stream, &capturing) == hipSuccess && capturing != hipStreamCaptureStatusNone)
    return fail(h, DSL_ERR_UNSUPPORTED, "step: emitters and sinks cannot act while the stream is being captured (clear them, or step outside the capture)");
  if (int rc = sources_refuse(h, "step")) return rc;
  if (look)
    if (int rc = sinks_apply(h, nullptr)) return rc;
  for (int e = 0; e < h->n_emitters; ++e) {
    if (!emitter_due(h, e, s)) continue;
    if ((long long)h->n + h->emit_m[e] > h->cap) {  // skipped whole, counted, not a layer
      h->src_skipped += 1;
      continue;
    }
    if (int rc = emit_layer(h, e)) return rc;
  }
  return DSL_OK;
}

int sources_option_set(dsl_handle* h, double value) {
  if (!(value >= 0.0 && value <= 1073741824.0) || value != std::floor(value))
    return fail(h, DSL_ERR_INVALID, "dsl_set_option: DSL_OPT_SINK_EVERY is a step count in [0, 2^30] (0: only dsl_particles_remove applies the sinks)");
  h->sink_every = (int)value;
  return DSL_OK;
}

int sources_option_get(dsl_handle* h, int option, double* value) {
  switch (option) {
    case DSL_OPT_EMITTERS: *value = (double)h->n_emitters; return DSL_OK;
    case DSL_OPT_SINKS: *value = (double)h->n_sinks; return DSL_OK;
    case DSL_OPT_EMITTED: *value = (double)h->src_emitted; return DSL_OK;
    case DSL_OPT_EMIT_SKIPPED: *value = (double)h->src_skipped; return DSL_OK;
    case DSL_OPT_REMOVED: *value = (double)h->src_removed; return DSL_OK;
    case DSL_OPT_SINK_EVERY: *value = (double)h->sink_every; return DSL_OK;
    default: return fail(h, DSL_ERR_INVALID, "dsl_get_option: unknown option");
  }
}

}  // namespace dsl

using namespace dsl;

int dsl_particles_append(dsl_handle* h, const float* host_positions, const float* host_velocities, size_t n_new) {
  CHECK_HANDLE(h);
  const std::string w = "dsl_particles_append";
  if (int rc = sources_refuse(h, w)) return rc;
  if (!host_positions || n_new == 0) return fail(h, DSL_ERR_INVALID, w + ": host_positions must not be NULL and n_new must be > 0");
  if (n_new > (size_t)(h->cap - h->n))
    return fail(h, DSL_ERR_NOMEM, w + ": dsl_params.capacity leaves no room (needs n_particles + n_new slots)");
  for (size_t k = 0; k < 3 * n_new; ++k)
    if (!std::isfinite(host_positions[k]) || (host_velocities && !std::isfinite(host_velocities[k])))
      return fail(h, DSL_ERR_INVALID, w + ": every position and velocity must be finite");
  // positions and velocities of a chunk share the staging array: 3 cap floats
  const size_t chunk = std::max<size_t>(1, (size_t)h->cap / 2);
  for (size_t at = 0; at < n_new; at += chunk) {
    const size_t m = std::min(chunk, n_new - at);
    float* xyz = h->stage;
    float* vxyz = host_velocities ? h->stage + 3 * m : nullptr;
    HIP_TRY(h, hipMemcpyAsync(xyz, host_positions + 3 * at, 3 * m * sizeof(float), hipMemcpyHostToDevice, h->stream));
    if (vxyz) HIP_TRY(h, hipMemcpyAsync(vxyz, host_velocities + 3 * at, 3 * m * sizeof(float), hipMemcpyHostToDevice, h->stream));
    if (int rc = emit_launch(h, (int)m, nullptr, EmitFace{}, xyz, vxyz)) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));  // (host pointers are not retained; the next chunk reuses the staging array)
  }
  return DSL_OK;
}

int dsl_emitter_add(dsl_handle* h, const dsl_emitter* e, int* id) {
  CHECK_HANDLE(h);
  const std::string w = "dsl_emitter_add";
  if (int rc = sources_refuse(h, w)) return rc;
  if (!e) return fail(h, DSL_ERR_INVALID, w + ": null emitter");
  if (h->n_emitters >= DSL_MAX_EMITTERS) return fail(h, DSL_ERR_INVALID, w + ": there are DSL_MAX_EMITTERS emitters already");
  if (e->nu < 1 || e->nv < 1 || (long long)e->nu * e->nv > (1ll << 20))
    return fail(h, DSL_ERR_INVALID, w + ": nu and nv must be >= 1 and nu * nv <= 2^20");
  if (e->period < 1) return fail(h, DSL_ERR_INVALID, w + ": period must be >= 1");
  if (e->first_step < 0 || e->max_layers < 0) return fail(h, DSL_ERR_INVALID, w + ": first_step and max_layers must be >= 0");
  if (e->shape != 0 && e->shape != 1) return fail(h, DSL_ERR_INVALID, w + ": shape is 0 (rectangle) or 1 (ellipse)");
  bool u0 = true, v0 = true;
  for (int c = 0; c < 3; ++c) {
    if (!std::isfinite(e->origin[c]) || !std::isfinite(e->u[c]) || !std::isfinite(e->v[c]) || !std::isfinite(e->velocity[c]))
      return fail(h, DSL_ERR_INVALID, w + ": every entry of origin, u, v and velocity must be finite");
    u0 = u0 && e->u[c] == 0.0f;
    v0 = v0 && e->v[c] == 0.0f;
  }
  if (u0 || v0) return fail(h, DSL_ERR_INVALID, w + ": u and v must not be all zero");
  // the kept points, b ascending and inside it a ascending, one word b * nu + a each
  std::vector<int> pts;
  const long long nu = e->nu, nv = e->nv;
  for (long long b = 0; b < nv; ++b)
    for (long long a = 0; a < nu; ++a) {
      const long long da = 2 * a - (nu - 1), db = 2 * b - (nv - 1);
      if (e->shape == 0 || da * da * nv * nv + db * db * nu * nu <= (nu * nv) * (nu * nv)) pts.push_back((int)(b * nu + a));
    }
  const int k = h->n_emitters;
  if (int rc = reserve(h, h->emit_pts[k], pts.size(), "dsl_emitter_add: the point list")) return rc;
  HIP_TRY(h, hipMemcpyAsync(h->emit_pts[k].p, pts.data(), pts.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  h->emitters[k] = *e;
  h->emit_m[k] = (int)pts.size();
  h->emit_layers[k] = 0;
  h->n_emitters = k + 1;
  if (id) *id = k;
  return DSL_OK;
}

int dsl_emitters_clear(dsl_handle* h) {
  CHECK_HANDLE(h);
  HIP_TRY(h, hipStreamSynchronize(h->stream));  // (a layer in flight still reads its list)
  for (int k = 0; k < DSL_MAX_EMITTERS; ++k) {
    h->dev_bytes -= h->emit_pts[k].count * sizeof(int);
    release(h->emit_pts[k]);
    h->emit_m[k] = 0;
    h->emit_layers[k] = 0;
  }
  h->n_emitters = 0;
  return DSL_OK;
}

int dsl_emit(dsl_handle* h, int emitter) {
  CHECK_HANDLE(h);
  const std::string w = "dsl_emit";
  if (int rc = sources_refuse(h, w)) return rc;
  if (emitter < 0 || emitter >= h->n_emitters) return fail(h, DSL_ERR_INVALID, w + ": unknown emitter id");
  if (h->emitters[emitter].max_layers != 0 && h->emit_layers[emitter] >= h->emitters[emitter].max_layers)
    return fail(h, DSL_ERR_INVALID, w + ": the emitter has emitted its max_layers layers");
  if ((long long)h->n + h->emit_m[emitter] > h->cap)
    return fail(h, DSL_ERR_NOMEM, w + ": the layer does not fit dsl_params.capacity");
  return emit_layer(h, emitter);
}

int dsl_sink_add(dsl_handle* h, const dsl_sink* s, int* id) {
  CHECK_HANDLE(h);
  const std::string w = "dsl_sink_add";
  if (int rc = sources_refuse(h, w)) return rc;
  if (!s) return fail(h, DSL_ERR_INVALID, w + ": null sink");
  if (h->n_sinks >= DSL_MAX_SINKS) return fail(h, DSL_ERR_INVALID, w + ": there are DSL_MAX_SINKS sinks already");
  for (int a = 0; a < 3; ++a)
    if (std::isnan(s->box_min[a]) || std::isnan(s->box_max[a]) || s->box_min[a] > s->box_max[a])
      return fail(h, DSL_ERR_INVALID, w + ": box_min and box_max must not be NaN, and box_min <= box_max on every axis");
  h->sinks[h->n_sinks] = *s;
  if (id) *id = h->n_sinks;
  h->n_sinks += 1;
  return DSL_OK;
}

int dsl_sinks_clear(dsl_handle* h) {
  CHECK_HANDLE(h);
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  h->n_sinks = 0;
  h->dev_bytes -= (h->src_ctr.count + h->src_scan.count) * sizeof(int);
  release(h->src_ctr);
  release(h->src_scan);
  return DSL_OK;
}

int dsl_particles_remove(dsl_handle* h, int64_t* removed) {
  CHECK_HANDLE(h);
  if (removed) *removed = 0;
  if (int rc = sources_refuse(h, "dsl_particles_remove")) return rc;
  return sinks_apply(h, removed);
}
