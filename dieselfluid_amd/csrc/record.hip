// record.hip -- the frame recorder: animation frames packed on the device during a run (dsl_recorder_set, dsl_record_now,
// dsl_record_poll / peek / release / read, and the step drivers' hook record_frame_due).  A translation unit of its own, so
// that every other unit's kernels come out as they are; its kernel list is tests/golden/device_kernels_record.txt.  Same
// flags as every unit: -ffp-contract=off keeps every operation at one rounding.  The rule is build-defined
// (include/dslsph.h) and restated operation for operation in tests/record_ref.py; it is the same in both
// math modes.
//
//   k_record_bounds   grid-stride over the slots: the captured particles (fluid, host index a multiple of the stride) with
//                     three finite coordinates, reduced per wave by shuffles, per workgroup through LDS, then one integer
//                     atomic max per workgroup and key -- the ordered key for a maximum, its complement for a minimum, so
//                     that seven zero words are the empty reduction -- and one integer add for the count
//   k_record_header   one wave: zeros into the planes' padding, and lane 0 the frame's 128-byte header into the staging frame, the keys back into floats, the box Q16
//                     is encoded against; the seven words go back to zero for the next frame
//   k_record_pack<Q>  one lane per slot: SoA loads and the id load coalesced, the write by host index a scatter of records of
//                     2 to 12 bytes into the staging frame (device memory: the host link gets one contiguous copy)
//
// Inside a skin episode the slot -> particle map is device state: the kernels take both id arrays and the SkinState and read
// ids[st->ids_sel & 1] themselves.  The recorder neither ends an episode nor keeps one from starting.
//
// Ordering, by events both ways: the pack of staging frame k is followed by ev_packed[k] on the step stream; the copy stream
// waits for it, copies the frame to its pinned slot and records ev_copied[k] and the slot's own event.  The step stream waits
// for ev_copied[k] before it packs into k again, and only if that copy is still outstanding -- with two staging frames in
// turn, that is when both are.  No host wait anywhere but in dsl_record_peek, for the one slot it hands out.
#include "engine.hpp"
#include "sph_device.hpp"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <new>

namespace dsl {

constexpr int kRecBlock = 256;
constexpr int kRecMaxGrid = 2048;  // workgroups of the bounds' grid-stride sweep: 7 atomics each
constexpr int kRecHeader = 128;    // bytes; every plane starts at a multiple of it
constexpr int kRecKeys = 8;        // words: [0..2] ~key of the minimum, [3..5] key of the maximum, [6] finite, [7] unused
constexpr unsigned int kRecMagic = 0x464C5344u;  // "DSLF"

// where a frame's planes lie (bytes from the frame's start; 0: no such plane)
struct FrameLayout {
  int m;
  size_t pos, vel, rho, bytes;
  size_t end[3];  // where the three planes' own bytes end (0: no such plane)
};

// what the header kernel writes and the pack kernel needs, by value
struct FrameArgs {
  unsigned long long frame_bytes;
  long long step;
  int n, m, stride, fields, encoding, auto_box;
  float box_min[3], box_max[3];
  float dt;
  unsigned int off_vel, off_rho;  // (a frame is below 2^32 bytes: 28 bytes per particle at the most, 2^31 particles)
  unsigned int pad_at[3], pad_len[3];  // the bytes between a plane's end and the next multiple of 128 (len 0: no such plane)
};

// the two slot -> particle maps and who says which is current: the device's SkinState inside a skin episode, else `sel`
struct IdMaps {
  const int *ids0, *ids1;
  const SkinState* st;
  int sel;
  __device__ __forceinline__ const int* current() const { return ((st != nullptr ? st->ids_sel : sel) & 1) ? ids1 : ids0; }
};

struct Recorder {
  dsl_recorder spec{};
  size_t slot_bytes = 0;  // dsl_record_frame_bytes(spec, capacity)
  int stages = 0;         // staging frames in device memory, taken in turn
  DevArray<unsigned char> stage[2];
  DevArray<unsigned int> keys;
  unsigned char* pinned = nullptr;  // slots x slot_bytes
  hipStream_t copy_stream = nullptr;
  hipEvent_t ev_packed[2] = {}, ev_copied[2] = {};
  bool copy_out[2] = {};  // a copy out of this staging frame was queued and not yet seen to have ended
  hipEvent_t ev_slot[64] = {};
  size_t slot_frame_bytes[64] = {};
  int head = 0, held = 0;  // the ring: the oldest unreleased slot, the unreleased slots
  int64_t seq = 0;         // frames recorded
  int64_t dropped = 0;
  hipEvent_t ev_time[4] = {};  // pack begin, pack end (step stream), copy begin, copy end (copy stream)
  bool timed_pack = false, timed_copy = false;
};

namespace {
inline size_t up128(size_t v) { return (v + (kRecHeader - 1)) & ~(size_t)(kRecHeader - 1); }

// the spec's own checks (nullptr: fine; else the message)
const char* spec_refusal(const dsl_recorder& s) {
  if (s.every < 1) return "every must be >= 1";
  if (s.stride < 1) return "stride must be >= 1";
  if (s.slots < 1 || s.slots > 64) return "slots must be 1 .. 64";
  if (s.first_step < 0) return "first_step must be >= 0";
  if (s.max_frames < 0) return "max_frames must be >= 0";
  if (s.fields & ~(DSL_REC_VELOCITY | DSL_REC_DENSITY)) return "fields has unknown bits (DSL_REC_VELOCITY | DSL_REC_DENSITY)";
  if (s.encoding != DSL_REC_F32 && s.encoding != DSL_REC_Q16) return "encoding is DSL_REC_F32 or DSL_REC_Q16";
  if (s.encoding == DSL_REC_Q16 && !s.auto_box)
    for (int a = 0; a < 3; ++a)
      if (!std::isfinite(s.box_min[a]) || !std::isfinite(s.box_max[a]) || s.box_min[a] > s.box_max[a])
        return "box_min and box_max must be finite with box_min <= box_max on every axis (or set auto_box)";
  return nullptr;
}

FrameLayout layout_of(const dsl_recorder& s, int n) {
  FrameLayout f{};
  f.m = (int)(((long long)n + s.stride - 1) / s.stride);
  const size_t m = (size_t)f.m, w = s.encoding == DSL_REC_Q16 ? 2 : 4;
  size_t at = kRecHeader;
  f.pos = at;
  at = up128(f.end[0] = at + 3 * w * m);
  if (s.fields & DSL_REC_VELOCITY) {
    f.vel = at;
    at = up128(f.end[1] = at + 3 * w * m);
  }
  if (s.fields & DSL_REC_DENSITY) {
    f.rho = at;
    at = up128(f.end[2] = at + w * m);
  }
  f.bytes = at;
  return f;
}
}  // namespace

// ---------------------------------------------------------------------------------------
// device side
// ---------------------------------------------------------------------------------------
namespace {
// the total order on float bits: negative numbers reversed below the positive ones, -0 just below +0
__device__ __forceinline__ unsigned int order_key(unsigned int bits) { return bits ^ ((bits >> 31) ? 0xffffffffu : 0x80000000u); }
__device__ __forceinline__ unsigned int key_bits(unsigned int key) { return key ^ ((key >> 31) ? 0x80000000u : 0xffffffffu); }
__device__ __forceinline__ bool finite_bits(unsigned int bits) { return (bits & 0x7fffffffu) < 0x7f800000u; }

__device__ __forceinline__ unsigned int wave_max(unsigned int v) {
#pragma unroll
  for (int off = kWave / 2; off >= 1; off >>= 1) v = max(v, (unsigned int)__shfl_xor((int)v, off));
  return v;
}

// float32 -> float16 bits, round to nearest even, in integer arithmetic: subnormal halves and overflow to infinity as IEEE
// 754 has them, whatever the conversion instruction's denormal mode is; a NaN keeps its sign and its ten top payload bits
// (0x7c01 where those are all zero) -- every float32 bit pattern comes out as numpy's astype(float16) has it
__device__ __forceinline__ unsigned int half_bits(unsigned int u) {
  const unsigned int sign = (u >> 16) & 0x8000u, a = u & 0x7fffffffu;
  if (a > 0x7f800000u) return sign | (((a >> 13) & 0x3ffu) ? (0x7c00u | ((a >> 13) & 0x3ffu)) : 0x7c01u);
  if (a >= 0x47800000u) return sign | 0x7c00u;  // 2^16 and beyond (65520 .. 2^16 gets there through the carry below)
  if (a >= 0x38800000u) {                       // a normal half: 2^-14 and beyond
    const unsigned int v = a - 0x38000000u;
    return sign | ((v + 0xfffu + ((v >> 13) & 1u)) >> 13);
  }
  if (a < 0x33000000u) return sign;  // below 2^-25: zero (2^-25 itself, the tie, goes to the even 0 below)
  const unsigned int shift = 126u - (a >> 23);  // 14 .. 24: the quotient counts units of 2^-24
  const unsigned int m = 0x800000u | (a & 0x7fffffu);
  const unsigned int q = m >> shift, rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1u);
  return sign | (q + ((rem > half || (rem == half && (q & 1u))) ? 1u : 0u));
}

// one coordinate against [lo, hi]: include/dslsph.h has the rule
__device__ __forceinline__ unsigned int q16(float x, float lo, float hi) {
  const float w = __fsub_rn(hi, lo);
  const float scale = (finite_bits(__float_as_uint(w)) && w > 0.0f) ? __fdiv_rn(65535.0f, w) : 0.0f;
  const float r = rintf(__fmul_rn(__fsub_rn(x, lo), scale));
  return r >= 65535.0f ? 65535u : (r > 0.0f ? (unsigned int)r : 0u);
}
}  // namespace

__global__ __launch_bounds__(kRecBlock) void k_record_bounds(int n_slots, int n, int stride, CSoa3 p, IdMaps maps,
                                                             unsigned int* __restrict__ keys) {
  __shared__ unsigned int s_red[kRecBlock / kWave][7];
  const int* __restrict__ ids = maps.current();
  unsigned int lo[3] = {0u, 0u, 0u}, hi[3] = {0u, 0u, 0u};  // (~key of the minimum, key of the maximum: 0 is "none yet")
  int found = 0;
  for (int base = blockIdx.x * kRecBlock; base < n_slots; base += gridDim.x * kRecBlock) {  // (uniform trips)
    const int s = base + threadIdx.x;
    bool take = false;
    unsigned int b[3] = {0u, 0u, 0u};
    if (s < n_slots) {
      const int id = ids[s];
      if ((unsigned int)id < (unsigned int)n && id % stride == 0) {
        b[0] = __float_as_uint(p.x[s]);
        b[1] = __float_as_uint(p.y[s]);
        b[2] = __float_as_uint(p.z[s]);
        take = finite_bits(b[0]) && finite_bits(b[1]) && finite_bits(b[2]);
      }
    }
    if (take) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const unsigned int k = order_key(b[c]);
        lo[c] = max(lo[c], ~k);
        hi[c] = max(hi[c], k);
      }
    }
    found += __popcll(__ballot(take));
  }
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    lo[c] = wave_max(lo[c]);
    hi[c] = wave_max(hi[c]);
  }
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      s_red[wave][c] = lo[c];
      s_red[wave][3 + c] = hi[c];
    }
    s_red[wave][6] = (unsigned int)found;
  }
  lds_barrier();
  if (threadIdx.x < 7) {
    unsigned int all = 0u, v = 0u;
#pragma unroll
    for (int w = 0; w < kRecBlock / kWave; ++w) {
      all += s_red[w][6];
      v = threadIdx.x < 6 ? max(v, s_red[w][threadIdx.x]) : v + s_red[w][6];
    }
    if (all != 0u) {  // (a workgroup that met no finite particle has nothing to say)
      if (threadIdx.x < 6) atomicMax(&keys[threadIdx.x], v);
      else atomicAdd(&keys[6], v);
    }
  }
}

__global__ __launch_bounds__(kWave) void k_record_header(FrameArgs a, unsigned int* keys, unsigned int* __restrict__ hdr) {
  // the planes' padding reads zero whatever an earlier frame with another count left there: under 128 bytes each, even
  unsigned char* frame = reinterpret_cast<unsigned char*>(hdr);
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (2u * threadIdx.x < a.pad_len[k]) reinterpret_cast<unsigned short*>(frame + a.pad_at[k])[threadIdx.x] = 0;
  if (threadIdx.x != 0) return;
  const unsigned int finite = keys[6];
  unsigned int bmin[3], bmax[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    bmin[c] = finite ? key_bits(~keys[c]) : 0x7f800000u;      // +inf
    bmax[c] = finite ? key_bits(keys[3 + c]) : 0xff800000u;   // -inf
  }
#pragma unroll
  for (int k = 0; k < 7; ++k) keys[k] = 0u;
  hdr[0] = kRecMagic;
  hdr[1] = (unsigned int)kRecHeader;
  hdr[2] = (unsigned int)(a.frame_bytes & 0xffffffffull);
  hdr[3] = (unsigned int)(a.frame_bytes >> 32);
  hdr[4] = (unsigned int)((unsigned long long)a.step & 0xffffffffull);
  hdr[5] = (unsigned int)((unsigned long long)a.step >> 32);
  hdr[6] = (unsigned int)a.n;
  hdr[7] = (unsigned int)a.m;
  hdr[8] = (unsigned int)a.stride;
  hdr[9] = (unsigned int)a.fields;
  hdr[10] = (unsigned int)a.encoding;
  hdr[11] = (unsigned int)a.auto_box;
  const bool q = a.encoding == DSL_REC_Q16;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    hdr[12 + c] = !q ? 0u : (a.auto_box ? bmin[c] : __float_as_uint(a.box_min[c]));
    hdr[15 + c] = !q ? 0u : (a.auto_box ? bmax[c] : __float_as_uint(a.box_max[c]));
    hdr[18 + c] = bmin[c];
    hdr[21 + c] = bmax[c];
  }
  hdr[24] = __float_as_uint(a.dt);
  hdr[25] = finite;
#pragma unroll
  for (int k = 26; k < 32; ++k) hdr[k] = 0u;
}

template <bool Q16>
__global__ __launch_bounds__(kRecBlock) void k_record_pack(int n_slots, FrameArgs a, CSoa3 p, CSoa3 v, const float* __restrict__ rho,
                                                           IdMaps maps, unsigned char* __restrict__ frame) {
  const int s = blockIdx.x * kRecBlock + threadIdx.x;
  if (s >= n_slots) return;
  const int id = maps.current()[s];
  if ((unsigned int)id >= (unsigned int)a.n || id % a.stride != 0) return;  // (a boundary particle, or not a captured one)
  const size_t m = (size_t)(id / a.stride);                                 // (< a.m: the staging frame is sized for it)
  const float x[3] = {p.x[s], p.y[s], p.z[s]};
  if (Q16) {
    const float* box = reinterpret_cast<const float*>(frame + 48);  // (what k_record_header left: lo[3], hi[3])
    unsigned short* o = reinterpret_cast<unsigned short*>(frame + kRecHeader) + 3 * m;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = (unsigned short)q16(x[c], box[c], box[3 + c]);
    if (a.fields & DSL_REC_VELOCITY) {  // (uniform)
      unsigned short* ov = reinterpret_cast<unsigned short*>(frame + a.off_vel) + 3 * m;
      ov[0] = (unsigned short)half_bits(__float_as_uint(v.x[s]));
      ov[1] = (unsigned short)half_bits(__float_as_uint(v.y[s]));
      ov[2] = (unsigned short)half_bits(__float_as_uint(v.z[s]));
    }
    if (a.fields & DSL_REC_DENSITY)
      reinterpret_cast<unsigned short*>(frame + a.off_rho)[m] = (unsigned short)half_bits(__float_as_uint(rho[s]));
  } else {
    float* o = reinterpret_cast<float*>(frame + kRecHeader) + 3 * m;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = x[c];
    if (a.fields & DSL_REC_VELOCITY) {
      float* ov = reinterpret_cast<float*>(frame + a.off_vel) + 3 * m;
      ov[0] = v.x[s];
      ov[1] = v.y[s];
      ov[2] = v.z[s];
    }
    if (a.fields & DSL_REC_DENSITY) reinterpret_cast<float*>(frame + a.off_rho)[m] = rho[s];
  }
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
namespace {
inline int rec_blocks(int n) { return (n + kRecBlock - 1) / kRecBlock; }

void recorder_destroy(dsl_handle* h) {
  Recorder* r = h->rec;
  if (!r) return;
  if (r->copy_stream) (void)hipStreamSynchronize(r->copy_stream);
  for (auto& a : r->stage) {
    h->dev_bytes -= a.count;
    release(a);
  }
  h->dev_bytes -= r->keys.count * sizeof(unsigned int);
  release(r->keys);
  if (r->pinned) (void)hipHostFree(r->pinned);
  for (int k = 0; k < 2; ++k) {
    if (r->ev_packed[k]) (void)hipEventDestroy(r->ev_packed[k]);
    if (r->ev_copied[k]) (void)hipEventDestroy(r->ev_copied[k]);
  }
  for (hipEvent_t e : r->ev_slot)
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : r->ev_time)
    if (e) (void)hipEventDestroy(e);
  if (r->copy_stream) (void)hipStreamDestroy(r->copy_stream);
  delete r;
  h->rec = nullptr;
}

// what a handle cannot record from: dsl_last_error names what is in the way
int record_refuse(dsl_handle* h, const std::string& w) {
  if (h->c.slab_axis >= 0 || h->c.n_ptr)
    return fail(h, DSL_ERR_UNSUPPORTED, w + ": a frame recorder is not supported in slab mode (leave it with dsl_slab_config(axis = -1) first)");
  if (h->ids_global) return fail(h, DSL_ERR_UNSUPPORTED, w + ": host order is gone after dsl_set_ids");
  return DSL_OK;
}

// One frame of the current state, stamped `step`: into the next staging frame on the step stream, from there to the ring's
// next slot on the copy stream.  The caller has found a released slot
int capture(dsl_handle* h, int64_t step) {
  Recorder* r = h->rec;
  const dsl_recorder& sp = r->spec;
  const int n_slots = h->n, n = n_fluid_of(h);
  const FrameLayout f = layout_of(sp, n);
  const int k = (int)(r->seq % r->stages), slot = (r->head + r->held) % sp.slots;
  if (r->copy_out[k]) {  // (the copy of `stages` frames ago: still on its way only when the host link is behind by all of them)
    if (hipEventQuery(r->ev_copied[k]) != hipSuccess) HIP_TRY(h, hipStreamWaitEvent(h->stream, r->ev_copied[k], 0));
    (void)hipGetLastError();  // (hipErrorNotReady is no error of ours)
    r->copy_out[k] = false;
  }
  FrameArgs a{};
  a.frame_bytes = f.bytes;
  a.step = step;
  a.n = n, a.m = f.m, a.stride = sp.stride, a.fields = sp.fields, a.encoding = sp.encoding;
  a.auto_box = (sp.encoding == DSL_REC_Q16 && sp.auto_box) ? 1 : 0;  // (the header says what was done: no box for F32)
  for (int c = 0; c < 3; ++c) a.box_min[c] = sp.box_min[c], a.box_max[c] = sp.box_max[c];
  a.dt = h->c.dt;
  a.off_vel = (unsigned int)f.vel, a.off_rho = (unsigned int)f.rho;
  for (int c = 0; c < 3; ++c) a.pad_at[c] = (unsigned int)f.end[c], a.pad_len[c] = (unsigned int)(up128(f.end[c]) - f.end[c]);
  const IdMaps maps{h->ids[0], h->ids[1], h->skin_live ? h->skin_state : nullptr, h->cur_ids};
  unsigned char* frame = r->stage[k].p;
  const bool clock = h->timing == 1;
  if (clock) {
    for (hipEvent_t& e : r->ev_time)
      if (!e) HIP_TRY(h, hipEventCreate(&e));
    HIP_TRY(h, hipEventRecord(r->ev_time[0], h->stream));
  }
  hipLaunchKernelGGL(k_record_bounds, dim3((unsigned)std::min(rec_blocks(n_slots), kRecMaxGrid)), dim3(kRecBlock), 0, h->stream, n_slots, n,
                     sp.stride, cpos(h), maps, r->keys.p);
  hipLaunchKernelGGL(k_record_header, dim3(1), dim3(kWave), 0, h->stream, a, r->keys.p, reinterpret_cast<unsigned int*>(frame));
  const dim3 g((unsigned)rec_blocks(n_slots)), b(kRecBlock);
  if (sp.encoding == DSL_REC_Q16)
    hipLaunchKernelGGL(k_record_pack<true>, g, b, 0, h->stream, n_slots, a, cpos(h), cvel(h), (const float*)h->rho, maps, frame);
  else
    hipLaunchKernelGGL(k_record_pack<false>, g, b, 0, h->stream, n_slots, a, cpos(h), cvel(h), (const float*)h->rho, maps, frame);
  HIP_TRY(h, hipGetLastError());
  if (clock) HIP_TRY(h, hipEventRecord(r->ev_time[1], h->stream));
  r->timed_pack = clock;
  HIP_TRY(h, hipEventRecord(r->ev_packed[k], h->stream));
  HIP_TRY(h, hipStreamWaitEvent(r->copy_stream, r->ev_packed[k], 0));
  if (clock) HIP_TRY(h, hipEventRecord(r->ev_time[2], r->copy_stream));
  HIP_TRY(h, hipMemcpyAsync(r->pinned + (size_t)slot * r->slot_bytes, frame, f.bytes, hipMemcpyDeviceToHost, r->copy_stream));
  if (clock) HIP_TRY(h, hipEventRecord(r->ev_time[3], r->copy_stream));
  r->timed_copy = clock;
  HIP_TRY(h, hipEventRecord(r->ev_copied[k], r->copy_stream));
  HIP_TRY(h, hipEventRecord(r->ev_slot[slot], r->copy_stream));
  r->copy_out[k] = true;
  r->slot_frame_bytes[slot] = f.bytes;
  r->held += 1;
  r->seq += 1;
  return DSL_OK;
}

// is the caller's stream being captured into a graph of its own?  (asked exactly as sources_step asks)
bool stream_capturing(dsl_handle* h) {
  hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing(h->stream, &capturing) == hipSuccess && capturing != hipStreamCaptureStatusNone;
}

// unreleased frames, from the oldest on, whose copy has landed
int64_t frames_ready(Recorder* r) {
  int64_t ready = 0;
  for (int i = 0; i < r->held; ++i) {
    if (hipEventQuery(r->ev_slot[(r->head + i) % r->spec.slots]) != hipSuccess) break;  // (FIFO on one stream: none behind it has)
    ready += 1;
  }
  (void)hipGetLastError();
  return ready;
}
}  // namespace

void record_free(dsl_handle* h) { recorder_destroy(h); }

int record_frame_due(dsl_handle* h) {
  Recorder* r = h->rec;
  const dsl_recorder& sp = r->spec;
  const int64_t s = h->steps;
  if (s < sp.first_step || (s - sp.first_step) % sp.every != 0) return DSL_OK;
  if (sp.max_frames != 0 && r->seq >= sp.max_frames) return DSL_OK;
  if (stream_capturing(h))
    return fail(h, DSL_ERR_UNSUPPORTED, "step: the recorder cannot take a frame while the stream is being captured (dsl_recorder_set(NULL), or step outside the capture)");
  if (int rc = record_refuse(h, "step")) return rc;
  if (r->held >= sp.slots) {  // dropped whole, counted, not a frame
    r->dropped += 1;
    return DSL_OK;
  }
  return capture(h, s);
}

int record_sync(dsl_handle* h) {
  if (h->rec) HIP_TRY(h, hipStreamSynchronize(h->rec->copy_stream));
  return DSL_OK;
}

int record_option_get(dsl_handle* h, int option, double* value) {
  Recorder* r = h->rec;
  *value = 0.0;
  if (!r) return DSL_OK;
  switch (option) {
    case DSL_OPT_RECORD_FRAMES: *value = (double)r->seq; return DSL_OK;
    case DSL_OPT_RECORD_DROPPED: *value = (double)r->dropped; return DSL_OK;
    case DSL_OPT_RECORD_READY: *value = (double)frames_ready(r); return DSL_OK;
    case DSL_OPT_RECORD_PACK_MS:
    case DSL_OPT_RECORD_COPY_MS: {
      const bool pack = option == DSL_OPT_RECORD_PACK_MS;
      if (!(pack ? r->timed_pack : r->timed_copy)) return DSL_OK;
      const int e0 = pack ? 0 : 2;
      float t = 0.f;
      hipError_t e = hipEventSynchronize(r->ev_time[e0 + 1]);
      if (e == hipSuccess) e = hipEventElapsedTime(&t, r->ev_time[e0], r->ev_time[e0 + 1]);
      if (e != hipSuccess) return fail(h, DSL_ERR_DEVICE, std::string("recorder time: ") + hipGetErrorString(e));
      *value = (double)t;
      return DSL_OK;
    }
    default: return fail(h, DSL_ERR_INVALID, "dsl_get_option: unknown option");
  }
}

}  // namespace dsl

using namespace dsl;

size_t dsl_record_frame_bytes(const dsl_recorder* spec, int n_particles) {
  if (!spec || n_particles < 1 || spec_refusal(*spec)) return 0;
  return layout_of(*spec, n_particles).bytes;
}

int dsl_recorder_set(dsl_handle* h, const dsl_recorder* spec) {
  CHECK_HANDLE(h);
  const std::string w = "dsl_recorder_set";
  if (spec) {
    if (const char* why = spec_refusal(*spec)) return fail(h, DSL_ERR_INVALID, w + ": " + why);
    if (int rc = record_refuse(h, w)) return rc;
  }
  HIP_TRY(h, hipStreamSynchronize(h->stream));  // (a frame being packed still reads the staging frames)
  recorder_destroy(h);
  if (!spec) return DSL_OK;
  Recorder* r = new (std::nothrow) Recorder();
  if (!r) return fail(h, DSL_ERR_NOMEM, w + ": out of host memory");
  h->rec = r;
  r->spec = *spec;
  r->slot_bytes = layout_of(*spec, h->cap - h->nb > 0 ? h->cap - h->nb : 1).bytes;
  // (on any failure below the handle stays usable, without a recorder)
  auto give_up = [&](int code, const std::string& msg) {
    recorder_destroy(h);
    (void)hipGetLastError();
    return fail(h, code, msg);
  };
  // two staging frames; one where the ring has a single slot (its frame is read before the next one finds the slot released)
  r->stages = std::min(2, (int)spec->slots);
  for (int k = 0; k < r->stages; ++k) {
    if (int rc = reserve(h, r->stage[k], r->slot_bytes, "dsl_recorder_set: a staging frame")) {
      const std::string msg = h->err;
      return give_up(rc, msg);
    }
  }
  if (int rc = reserve(h, r->keys, (size_t)kRecKeys, "dsl_recorder_set: the bounds' keys")) {
    const std::string msg = h->err;
    return give_up(rc, msg);
  }
  hipError_t e = hipMemsetAsync(r->keys.p, 0, kRecKeys * sizeof(unsigned int), h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&r->copy_stream, hipStreamNonBlocking);
  for (int k = 0; k < 2 && e == hipSuccess; ++k) {
    e = hipEventCreateWithFlags(&r->ev_packed[k], hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&r->ev_copied[k], hipEventDisableTiming);
  }
  for (int k = 0; k < spec->slots && e == hipSuccess; ++k) e = hipEventCreateWithFlags(&r->ev_slot[k], hipEventDisableTiming);
  if (e != hipSuccess) return give_up(DSL_ERR_DEVICE, w + ": " + hipGetErrorString(e));
  e = hipHostMalloc((void**)&r->pinned, (size_t)spec->slots * r->slot_bytes, hipHostMallocDefault);
  if (e != hipSuccess) {
    r->pinned = nullptr;
    return give_up(DSL_ERR_NOMEM, w + ": hipHostMalloc of the slots: " + hipGetErrorString(e));
  }
  return DSL_OK;
}

int dsl_record_now(dsl_handle* h) {
  CHECK_HANDLE(h);
  const std::string w = "dsl_record_now";
  Recorder* r = h->rec;
  if (!r) return fail(h, DSL_ERR_INVALID, w + ": no recorder is set (dsl_recorder_set)");
  if (int rc = record_refuse(h, w)) return rc;
  if (stream_capturing(h)) return fail(h, DSL_ERR_UNSUPPORTED, w + ": not while the stream is being captured");
  if (r->spec.max_frames != 0 && r->seq >= r->spec.max_frames)
    return fail(h, DSL_ERR_INVALID, w + ": the recorder has recorded its max_frames frames");
  if (r->held >= r->spec.slots) return fail(h, DSL_ERR_NOMEM, w + ": no slot is released (dsl_record_release, dsl_record_read)");
  return capture(h, h->steps);
}

int dsl_record_poll(dsl_handle* h, int64_t* recorded, int64_t* ready, int64_t* dropped) {
  CHECK_HANDLE_ONLY(h);
  Recorder* r = h->rec;
  if (recorded) *recorded = r ? r->seq : 0;
  if (ready) *ready = r ? frames_ready(r) : 0;
  if (dropped) *dropped = r ? r->dropped : 0;
  return DSL_OK;
}

int dsl_record_peek(dsl_handle* h, const void** frame, size_t* bytes) {
  CHECK_HANDLE_ONLY(h);
  Recorder* r = h->rec;
  if (!frame) return fail(h, DSL_ERR_INVALID, "dsl_record_peek: null output");
  if (!r || r->held == 0) return fail(h, DSL_ERR_INVALID, "dsl_record_peek: there is no unreleased frame");
  HIP_TRY(h, hipEventSynchronize(r->ev_slot[r->head]));
  *frame = r->pinned + (size_t)r->head * r->slot_bytes;
  if (bytes) *bytes = r->slot_frame_bytes[r->head];
  return DSL_OK;
}

int dsl_record_release(dsl_handle* h) {
  CHECK_HANDLE_ONLY(h);
  Recorder* r = h->rec;
  if (!r || r->held == 0) return fail(h, DSL_ERR_INVALID, "dsl_record_release: there is no unreleased frame");
  HIP_TRY(h, hipEventSynchronize(r->ev_slot[r->head]));  // (a slot whose copy is still on its way cannot take the next frame)
  r->head = (r->head + 1) % r->spec.slots;
  r->held -= 1;
  return DSL_OK;
}

int dsl_record_read(dsl_handle* h, void* host_out, size_t bytes) {
  CHECK_HANDLE_ONLY(h);
  const void* frame = nullptr;
  size_t have = 0;
  if (!host_out) return fail(h, DSL_ERR_INVALID, "dsl_record_read: null output");
  if (int rc = dsl_record_peek(h, &frame, &have)) return rc;
  if (bytes < have) return fail(h, DSL_ERR_INVALID, "dsl_record_read: bytes is smaller than the frame (dsl_record_frame_bytes)");
  std::memcpy(host_out, frame, have);
  return dsl_record_release(h);
}
