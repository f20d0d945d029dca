// engine.hpp -- what the host units of libdslsph.so share: the handle, the error and allocation helpers, the small
// accessors, and the declarations of the functions that cross a unit boundary.  Private to csrc/: the C ABI is
// include/dslsph.h.  It includes no kernel header (most of those define non-template __global__ functions, which a
// second unit would emit again), so any unit may include it; the units are
//   dslsph.hip         the engine: every kernel launch of the kernel headers, the passes, the single-GPU step drivers
//   collider_host.hip  the collider's host side (the kernels are in collide.hip, collide_index.hip, collide_slab.hip)
//   slab_link.hip      multi-GPU: communicator, slab link, re-balancing, the native slab step drivers
//   volume.hip         field volumes: dsl_field_volume and its two kernels (a host unit with kernels of its own)
//   surface.hip        fluid surfaces: dsl_surface_extract, dsl_field_surface and their four kernels (likewise)
//   surface_mesh.hip   the indexed mesh: dsl_surface_extract_indexed, dsl_field_surface_indexed and their three kernels
//   sdf.hip            implicit colliders: dsl_mesh_distance_volume, dsl_collider_set_volume, the volume collide pass, their kernels
//   sdf_rigid.hip      the volume collider in rigid motion: dsl_collider_volume_motion, dsl_collider_volume_impulse, their two kernels
//   bodies.hip         rigid bodies: dsl_body_*, several volume colliders in one pass, the fold that integrates their poses
//   contact.hip        their contact stage: dsl_contact_*, contact points, detection against the wall box and each other, the solve
//   sources.hip        sources and sinks: dsl_particles_append, dsl_emit*, dsl_sink*, dsl_particles_remove, their seven kernels
//   record.hip         the frame recorder: dsl_recorder_set, dsl_record_*, the step drivers' hook, their four kernels
// The seven before the last two are the lattice units; what they share is lattice.hpp (included here, since the handle holds its DevArray and
// PhaseClock members): the lattice and its one check, the collider's cell evaluation, the arrays that grow on demand and the
// per-phase event clocks.  The barrier with its LDS drain, the voxel coordinate and the ordered dot product are sph_device.hpp's.
#pragma once

#include "../../include/dslsph.h"

#include <hip/hip_runtime.h>

#include <string>
#include <utility>
#include <vector>

#include "collide.hpp"
#include "lattice.hpp"

struct SlabLink;

namespace dsl {
// the lists are built where the particles will be about half way through the lists' life: the fastest particle may use up
// this fraction of the displacement budget at the build itself (DSL_OPT_SKIN_PREDICT; 0: built where the particles are)
constexpr float kSkinPredict = 0.8f;
struct Recorder;  // record.hip
}  // namespace dsl

struct dsl_handle {
  int device = 0;
  hipStream_t own_stream = nullptr, stream = nullptr;
  dsl_params prm{};
  dsl::DevConsts c{};
  int n = 0, cap = 0, ncell = 0, ncell_pad = 0, nscan = 0;
  // boundary particles (particle_array.go:123-128): ids n_fluid .. n-1.  The reference's Get() reads
  // index == N() as the zero particle (particle_array.go:98,107), so the first boundary particle takes
  // part in every sum AT THE ORIGIN; the device copy holds (0,0,0) for it and b0_pos what was uploaded.
  int nb = 0;  // boundary particles; N() = n - nb (n itself changes in slab mode, where nb is always 0)
  float b0_pos[3] = {0.f, 0.f, 0.f};
  bool ids_global = false;  // dsl_set_ids replaced the host-order map
  int* dcounter = nullptr;
  // slab mode: [0] live particle count, [1..4] band counters (lo/hi full, lo/hi position-only),
  // [5] overflow high-water mark, [6],[7] largest full / position-only band counts seen
  int* dn = nullptr;
  int* pack_counts = nullptr;  // band selection: per-block record counts, then offsets (kernels_grid.hpp)
  // split slab step (dsl_force_pass_split): band tiles first, interior tiles after the pack
  float split_margin = 0.0f, split_width = 0.0f;
  bool split_pending = false;
  bool pci_split_guard = false;  // between DSL_PCI_BEGIN_STEP and DSL_PCI_END_STEP
  hipEvent_t ev_band = nullptr;
  // DSL_NEIGH_LSH_REF
  bool lsh = false;
  int lsh_bits = 0, lsh_cap = 0;
  float* hashv = nullptr;
  int *bucket_of = nullptr, *lsh_table = nullptr, *lsh_len = nullptr, *lsh_samples = nullptr;
  dsl::TileGrid tg{};
  int *tiles = nullptr, *n_tiles = nullptr;
  int *tile_desc_of = nullptr, *tile_desc = nullptr;  // per list entry: index of the tile's table; the tables (k_tile_desc)
  // SoA state
  float* pv[2][6] = {};
  int* ids[2] = {};
  float* frc[2][3] = {};
  float* pci[2][6] = {};
  float *rho = nullptr, *pterm = nullptr, *press = nullptr, *scratch1 = nullptr;
  float* gterm[3] = {};  // PCISPH: cached pressure-gradient force term
  // PCISPH with the DensityF query points in bins of their own (kernels_sph.hpp: k_pci_predict_bin): the histogram over
  // the particles' grid cells, its prefix, the scan's tile sums, one record per query, and the 512 drift counters the
  // un-binned kernels keep.  pci_bin_mode: 0 = the library switches when 0.2 % of the predicted positions have left their
  // particle's tile (looked at every kPciDriftPeriod steps; a one-way latch until the next dsl_pcisph_begin), 1 = always,
  // -1 = never (dsl_pcisph_set_binning; DSL_PCI_BINNED presets it)
  int pci_bin_mode = 0;
  int build_seq = 0;  // neighbour builds so far (k_cell_rank<true> stamps its off-grid flag with it)
  // the query histogram was handed to an iteration that may not have cleaned it again (the table builder / the scan do,
  // behind the predictor: an error return in between leaves it dirty -- the sort's sort_scratch_dirty, for the queries)
  bool qcount_dirty = false;
  bool pci_counters_clean = false;  // n_qtiles[0..1] are known to be zero (the first binned iteration clears them itself)
  bool pci_iter_pending = false;  // DSL_PCI_ITERATE without its DSL_PCI_CHECK yet (the check clears the iteration's counters)
  bool pci_binned = false;
  bool pci_qpair = true;   // ... two queries per lane (DSL_PCI_QPAIR=0: one)
  bool pci_qtiled = true;  // FAST: sweep the binned queries tile by tile out of LDS (DSL_PCI_QTILED=0: the global-memory sweep)
  int64_t pci_steps = 0;  // completed steps since dsl_pcisph_begin
  int *qcount = nullptr, *qstart = nullptr, *qsums = nullptr;
  int *qtiles = nullptr, *n_qtiles = nullptr, *qtile_desc = nullptr;  // FAST: the tiles that hold queries and their tables
  // FAST, two queries per lane: kQueryRow record slots per grid cell instead of the sorted array (no prefix scan, no
  // scatter pass: kernels_tiled.hpp, tile_setup_load_counts); DSL_PCI_QROWS=0, or an allocation that fails, keeps the array
  float4* qrows = nullptr;
  bool pci_qrows = true;
  // ... and the rows kept from one correction iteration to the next inside a step (k_pci_predict_bin<.., INCR>): qslot =
  // every particle's record index; pci_rows_live = this step's rows hold every query (its first iteration filled them)
  int* qslot = nullptr;
  bool pci_qincr = true;
  bool pci_rows_live = false;
  float4* qrec = nullptr;
  unsigned int* pci_drift = nullptr;
  unsigned int* pci_drift_host = nullptr;  // pinned: the snapshot of the counters the next look reads
  hipEvent_t ev_drift = nullptr;
  bool drift_pending = false;
  float* xsph[3] = {};   // build-defined XSPH correction of the current step (PCISPH path)
  unsigned int* nmask = nullptr;  // FAST: per-particle in-range masks from the density sweep (kMaskWords x cap)
  bool masks_valid = false;
  int *rank = nullptr, *cell_count = nullptr, *cell_start = nullptr, *block_sums = nullptr;
  // in-cell ordering of the counting sort (kernels_grid.hpp, k_scatter): bitmap of the cells to order,
  // their ids at the slots the atomic ranks name, one byte per particle that marks their particles
  unsigned int* unordered = nullptr;
  int *sort_keys = nullptr, *sort_work = nullptr;
  int* cell_keys = nullptr;  // kCellKeys ids per grid cell: the one-pass in-cell ordering (kernels_grid.hpp); DSL_OPT_CELL_KEYS = 0: nullptr
  int* cell_keys_alloc = nullptr;
  float* stage = nullptr;
  dsl::DevStats* dstats = nullptr;
  int cur_pv = 0, cur_ids = 0, cur_f = 0, cur_pci = 0;
  bool grid_valid = false, forces_uniform = false, press_zero = true, pci_active = false, dens_fresh = false;
  // dens_held: rho / pterm hold per-particle values in the CURRENT slot order (possibly stale ones: after a mass
  // change or new boundary particles the reference, too, keeps the old density on the same particle until the
  // next DensityAll), so a sort has to carry them.  dens_fresh: they also belong to the current positions / mass.
  bool dens_held = false;
  // the histogram / "cells to order" bitmap were handed to a build that may not have cleaned them again
  bool sort_scratch_dirty = false;
  // (a one-launch decoupled look-back scan was measured in round 3: 6 x SLOWER at 16.4M cells, 0.46 against 0.077 ms --
  // all 4004 tiles are resident at once, so the look-back is one long chain of agent-scope round trips through the
  // eight XCDs' separate L2s; profiles/README.md, r03.  Removed in round 4.)
  bool density_pair = true;  // FAST density with two targets per lane (DSL_DENSITY_PAIR=0: the lane-per-target kernel)
  int max_persistent_blocks = 0;  // DSL_PERSISTENT_BLOCKS (tests)
  int64_t steps = 0;
  size_t dev_bytes = 0;  // device memory this handle has allocated (DSL_OPT_DEVICE_BYTES)
  // the skin step (kernels_skin.hpp; DSL_OPT_SKIN): neighbour lists against h (1 + skin), walked until some particle may
  // have moved skin * h / 2.  skin_live: the device's SkinState is the authority on which slot -> particle map is current
  // and the grid's cells are h (1 + skin) wide -- every other entry point settles that first (skin_settle).
  float skin = 0.0f;
  bool skin_live = false;
  int64_t skin_steps_total = 0, skin_rebuilds_total = 0;  // of the skin episodes already settled
  bool skin_list_overflow = false;
  // the flow outran the skin (SkinState::give_up, looked at every kSkinLook steps): plain steps until step skin_retry_at
  int64_t skin_retry_at = 0, skin_live_steps = 0;
  int skin_suspensions = 0;
  int tile_box[3] = {8, 4, 4};
  int alloc_ntiles = 0;  // tiles the tile lists and tables were allocated for
  int tile_tbz = dsl::kTB;  // cell layers per tile along z (sph_device.hpp: TileGrid::tbz); 3 while the skin step owns the grid
  dsl::SkinState* skin_state = nullptr;
  uint4* lists = nullptr;
  float* pvz[6] = {};  // the sort's output set of a skin step (Z)
  float* pvr[3] = {};  // ... and the build's reference positions x + tau v in the same order (SkinState::tau)
  float skin_predict = dsl::kSkinPredict;  // DSL_OPT_SKIN_PREDICT
  bool list_build_lockstep = true;    // DSL_OPT_LIST_BUILD
  int grid_oversub = 8;               // DSL_OPT_GRID_OVERSUB
  // DSL_OPT_TILE_QUEUE: the single-domain tile kernels draw their tiles from per-XCD counters (kernels_tiled.hpp: TileFeed,
  // dynamic mode) instead of walking a share dealt in advance.  16 launch sites x 16 ints, left at zero by every launch.
  int tile_queue = 1;  // 0 never, 1 from 8M particles on, 2 always (tests)
  int* walk_ctr = nullptr;
  int walk_parity[16] = {};
  // triangle-mesh collider (kernels_collide.hpp; dsl_collider_set_mesh): col_tri = 0: none, nothing is launched
  int col_tri = 0, col_alloc = 0;
  float col_radius = 0.0f, col_rest = 0.0f, col_s_thr = -1.0f;
  bool col_cull = true;
  dsl::TriRec* col_rec = nullptr;
  dsl::TriBox *col_box = nullptr, *col_chunk = nullptr;
  int* col_hits = nullptr;    // particles the last collide pass moved
  float* col_query = nullptr; // dsl_collider_query's staging: tri, normal, coord, point in host order (10 words per particle)
  // the cell index over the triangles (kernels_collide_index.hpp; DSL_OPT_COLLIDE_INDEX): col_ix_cells = 0: none
  bool col_ix_on = false;
  float col_ix_edge_req = 0.0f;  // DSL_OPT_COLLIDE_INDEX_EDGE; 0: the library's choice
  dsl::ColIndex col_ix{};
  int col_ix_cells = 0;
  long long col_ix_entries = 0;
  size_t col_ix_bytes = 0;         // its share of dev_bytes
  bool col_last_indexed = false;   // the last collide pass or query ran the indexed kernel
  // a mesh on a slab handle (DSL_OPT_COLLIDE_SLAB; csrc/collide_slab.hip).  col_stage: what the last integrate wrote and
  // nobody has collided, packed or re-sorted since -- 0 nothing (dsl_collide_pass is refused), 1 everything (dsl_force_pass,
  // Update), 2 the band layers into the output half (DSL_SPLIT_BAND), 3 the other layers (DSL_SPLIT_INNER).
  // col_step_zeroed: the hit and visit counters were zeroed since the last neighbour build (they sum over a step's launches)
  bool col_slab = false;
  int col_stage = 0;
  bool col_step_zeroed = false;
  // field volumes (volume.hip; dsl_field_volume).  vol_stage: the library's own output array of a host_out-only call (grows on
  // demand); vol_ctr: LDS / fallback / empty bricks and staged records of the last brick launch; vol_last_bricks: the last call ran the brick form
  dsl::DevArray<float> vol_stage;
  unsigned long long* vol_ctr = nullptr;
  bool vol_bricks = true;  // DSL_OPT_VOLUME_BRICKS (the measured choice: DESIGN.md 4.3)
  bool vol_last_bricks = false;
  // fluid surfaces (surface.hip; dsl_surface_extract).  surf_scan: one 64-bit count, then offset, per brick of 8 x 8 x 4 cubes and
  // the scan's upper levels behind them; surf_ctr: [0] triangles T, [1] bricks with a triangle, of the last call; surf_stage:
  // dsl_field_surface's triangles before they go to the host.  All three allocated on first use and grown on demand.
  // surf_clock: the last call's phases count, scan and emit
  dsl::DevArray<unsigned long long> surf_scan;
  unsigned long long* surf_ctr = nullptr;
  dsl::DevArray<float> surf_stage;
  dsl::PhaseClock<3> surf_clock;
  // the indexed mesh (surface_mesh.hip; dsl_surface_extract_indexed).  mesh_words: one word per voxel, the voxel's vertex
  // prefix inside its brick of 8 x 8 x 4 voxels << 7 | its 7-bit edge mask; mesh_scan: count, then offset, per voxel brick and
  // the scan's upper levels; mesh_ctr: [0] vertices V of the last call; mesh_stage: dsl_field_surface_indexed's positions,
  // normals and indices before they go to the host.  mesh_clock: the phases vertex count, scan, vertex emit and index emit
  dsl::DevArray<unsigned int> mesh_words;
  dsl::DevArray<unsigned long long> mesh_scan;
  unsigned long long* mesh_ctr = nullptr;
  dsl::DevArray<float> mesh_stage;
  dsl::PhaseClock<4> mesh_clock;
  // distance volumes of a mesh (sdf.hip; dsl_mesh_distance_volume), all allocated on first use and grown on demand.  sdf_stage:
  // the output of a host_out-only call; sdf_verts: the caller's vertices; sdf_rec / sdf_box: four float4 and six floats per
  // triangle; sdf_scan: one count, then offset, per brick of 8 x 8 x 4 voxels and the scan's upper levels; sdf_list: the
  // bricks' triangle lists; sdf_marks: one word per voxel, the sign sweep's marks; sdf_ctr: [0] bricks with a list, [1] triangle
  // visits, [2] list entries of the last call.  sdf_clock: the phases distance and sign
  dsl::DevArray<float> sdf_stage, sdf_verts, sdf_box;
  dsl::DevArray<float4> sdf_rec;
  dsl::DevArray<unsigned long long> sdf_scan;
  dsl::DevArray<int> sdf_list;
  dsl::DevArray<unsigned int> sdf_marks;
  unsigned long long* sdf_ctr = nullptr;
  dsl::PhaseClock<2> sdf_clock;
  // the volume collider (sdf.hip; dsl_collider_set_volume): the library's copy of the volume and its lattice.  colv_on: set --
  // the collide pass runs k_collide_volume and a mesh is refused; colv_query: dsl_collider_volume_query's staging (4 words per particle)
  dsl::DevArray<float> colv_vol;
  bool colv_on = false;
  dsl::Lattice colv_g{};
  float colv_radius = 0.0f, colv_rest = 0.0f;
  int colv_flags = 0;
  float* colv_query = nullptr;
  // ... in rigid motion (sdf_rigid.hip; dsl_collider_volume_motion).  colv_moving: a motion is set -- the collide pass and the
  // query run k_collide_volume_rigid with these 18 numbers by value; colv_partial: six sums per workgroup of the last pass,
  // component-major; colv_acc: impulse and torque impulse since the last reset.  Both allocated when a motion is first set
  bool colv_moving = false;
  float colv_rot[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
  float colv_trans[3] = {}, colv_lin[3] = {}, colv_ang[3] = {};
  dsl::DevArray<float> colv_partial;
  float* colv_acc = nullptr;
  // rigid bodies (bodies.hip; dsl_body_add): n_bodies = 0: none, nothing is launched.  body_rec: DSL_MAX_BODIES records in
  // device memory (volume pointer, lattice, props, state, R, accumulators), written by the host calls and by the fold's
  // integration; body_vol: the library's copies of the volumes; body_partial: six sums per workgroup and body of the last
  // pass, [body][component][workgroup]; body_query: dsl_body_query's staging (4 words per particle)
  int n_bodies = 0;
  bool bodies_integrate = true;  // DSL_OPT_BODIES_INTEGRATE
  dsl::DevArray<unsigned char> body_rec;
  dsl::DevArray<float> body_vol[DSL_MAX_BODIES];
  dsl::DevArray<float> body_partial;
  float* body_query = nullptr;
  // their contact stage (contact.hip; DSL_OPT_BODIES_CONTACT): nothing below is allocated while the option is 0 and no
  // dsl_contact_* call was made.  body_g: the bodies' lattices as dsl_body_add checked them; contact_pts / contact_m: a body's
  // contact points (voxel indices, ascending) and their number, bit b of contact_built: body b's list exists; contact_scan:
  // the list build's counts, then offsets, per 256 voxels; contact_meta: one record per body and the block table of the
  // detection's flattened grid, laid out for contact_k bodies (0: stale); contact_partial: nine words per workgroup and
  // target; contact_table: E, 9 K (6 + K) words, contact_table_k: the K of the last detection (0: none yet); contact_ctr:
  // the entries of the last solve that got past k > 0
  int bodies_contact = 0;
  dsl::Lattice body_g[DSL_MAX_BODIES] = {};
  dsl::DevArray<int> contact_pts[DSL_MAX_BODIES];
  int contact_m[DSL_MAX_BODIES] = {};
  unsigned contact_built = 0;
  dsl::DevArray<int> contact_scan;
  dsl::DevArray<unsigned char> contact_meta;
  int contact_k = 0, contact_blocks = 0, contact_table_k = 0;
  dsl::DevArray<float> contact_partial, contact_table;
  dsl::DevArray<int> contact_ctr;
  // sources and sinks (sources.hip; dsl_emitter_add, dsl_sink_add): nothing below is allocated, and no step launches
  // anything for it, while there is no emitter, no sink and none of the calls was made.  emit_pts / emit_m: an emitter's
  // kept lattice points, b * nu + a each, in layer order, and their number; emit_layers: the layers it has emitted;
  // src_ctr: the sink count's word; src_scan: the compaction's counts, then offsets, per 256 host indices and the total
  // behind them.  count_changed: an append, an emission or a removal has changed the particle count of this handle
  int n_emitters = 0, n_sinks = 0;
  dsl_emitter emitters[DSL_MAX_EMITTERS] = {};
  dsl::DevArray<int> emit_pts[DSL_MAX_EMITTERS];
  int emit_m[DSL_MAX_EMITTERS] = {};
  int64_t emit_layers[DSL_MAX_EMITTERS] = {};
  dsl_sink sinks[DSL_MAX_SINKS] = {};
  int sink_every = 8;  // DSL_OPT_SINK_EVERY
  int64_t src_emitted = 0, src_skipped = 0, src_removed = 0;
  bool count_changed = false;
  dsl::DevArray<int> src_ctr, src_scan;
  // the frame recorder (record.hip; dsl_recorder_set): nullptr: none -- no launch, no allocation, no step looks further
  dsl::Recorder* rec = nullptr;
  std::string err;
  SlabLink* link = nullptr;  // dsl_slab_attach: the slab's RCCL link to its neighbours (slab_link.hip)
  // timing
  int timing = 0;  // 0 off, 1 every kernel, 2 the step's dominant kernels only
  std::vector<hipEvent_t> pool;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pending[DSL_K_END];
  double total_ms[DSL_K_END] = {};
  int64_t launches[DSL_K_END] = {};
};

namespace dsl {

int fail(dsl_handle* h, int code, const std::string& msg);  // h == nullptr: the message of dsl_last_error(NULL)

#define HIP_TRY(h, expr)                                                                             \
  do {                                                                                               \
    hipError_t e__ = (expr);                                                                         \
    if (e__ != hipSuccess)                                                                           \
      return fail((h), DSL_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e__));          \
  } while (0)

#define CHECK_HANDLE_ONLY(h)                              \
  do {                                                    \
    if (!(h)) return fail(nullptr, DSL_ERR_INVALID, "null handle"); \
    hipError_t e__ = hipSetDevice((h)->device);           \
    if (e__ != hipSuccess) return fail((h), DSL_ERR_DEVICE, std::string("hipSetDevice: ") + hipGetErrorString(e__)); \
  } while (0)
int skin_settle(dsl_handle* h);
// every entry point but the step driver itself first brings a handle that is in the middle of skin steps back to the
// plain state (one small device read: kernels_skin.hpp)
#define CHECK_HANDLE(h)                                   \
  do {                                                    \
    CHECK_HANDLE_ONLY(h);                                 \
    if ((h)->skin_live)                                   \
      if (int rc__ = skin_settle(h)) return rc__;         \
  } while (0)

// number of slots a per-particle launch has to cover: exact without slabs; in slab mode the
// live count lives on the device, so cover the whole capacity (idle blocks exit at once)
inline int launch_n(const dsl_handle* h) { return h->c.n_ptr ? h->cap : h->n; }

template <class T>
int dev_alloc(dsl_handle* h, T** p, size_t count) {
  // (64 bytes of padding: the staging quads of the tiled kernels read up to three elements past a row, the ordered
  // scatter up to seven keys past a cell)
  hipError_t e = hipMalloc((void**)p, count * sizeof(T) + 64);
  if (e != hipSuccess) return fail(h, DSL_ERR_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
  // Every array starts from zeros (NewParticleArray zero-fills its slices too, particle_array.go:18-33): hipMalloc hands
  // out whatever the previous owner left, and nothing a run computes may depend on that -- neither the padding the
  // unaligned staging quads read past a row nor a plane that is only written for some particles.  Once per handle.
  e = hipMemsetAsync(*p, 0, count * sizeof(T) + 64, h->stream);
  if (e != hipSuccess) return fail(h, DSL_ERR_DEVICE, std::string("hipMemsetAsync: ") + hipGetErrorString(e));
  h->dev_bytes += count * sizeof(T) + 64;
  return DSL_OK;
}

hipEvent_t get_event(dsl_handle* h);

template <class F>
int timed(dsl_handle* h, int kid, F&& launch) {
  if (h->timing == 1 || (h->timing == 2 && (kid == DSL_K_DENSITY || kid == DSL_K_FORCE_INTEGRATE || kid == DSL_K_PCI_DENSITY))) {
    hipEvent_t a = get_event(h), b = get_event(h);
    (void)hipEventRecord(a, h->stream);
    launch();
    (void)hipEventRecord(b, h->stream);
    h->pending[kid].emplace_back(a, b);
  } else {
    launch();
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(h, DSL_ERR_DEVICE, std::string("kernel launch: ") + hipGetErrorString(e));
  return DSL_OK;
}

inline CSoa3 cpos(dsl_handle* h) { return {h->pv[h->cur_pv][0], h->pv[h->cur_pv][1], h->pv[h->cur_pv][2]}; }
inline CSoa3 cvel(dsl_handle* h) { return {h->pv[h->cur_pv][3], h->pv[h->cur_pv][4], h->pv[h->cur_pv][5]}; }
inline Soa3 mpos(dsl_handle* h, int w) { return {h->pv[w][0], h->pv[w][1], h->pv[w][2]}; }
inline Soa3 mvel(dsl_handle* h, int w) { return {h->pv[w][3], h->pv[w][4], h->pv[w][5]}; }
inline Soa3 mfrc(dsl_handle* h) { return {h->frc[h->cur_f][0], h->frc[h->cur_f][1], h->frc[h->cur_f][2]}; }
inline CSoa3 cfrc(dsl_handle* h) { return {h->frc[h->cur_f][0], h->frc[h->cur_f][1], h->frc[h->cur_f][2]}; }
inline Soa3 mpcip(dsl_handle* h) { return {h->pci[h->cur_pci][0], h->pci[h->cur_pci][1], h->pci[h->cur_pci][2]}; }
inline Soa3 mpciv(dsl_handle* h) { return {h->pci[h->cur_pci][3], h->pci[h->cur_pci][4], h->pci[h->cur_pci][5]}; }
inline Soa3 mxsph(dsl_handle* h) { return {h->xsph[0], h->xsph[1], h->xsph[2]}; }
inline Soa3 mgterm(dsl_handle* h) { return {h->gterm[0], h->gterm[1], h->gterm[2]}; }
constexpr Soa3 kNoSoa3{nullptr, nullptr, nullptr};
inline CSoa3 as_const(Soa3 a) { return {a.x, a.y, a.z}; }
// the PCISPH predictor state, or three nulls while PCISPH is not running
inline Soa3 mpcip_if_active(dsl_handle* h) { return h->pci_active ? mpcip(h) : kNoSoa3; }
inline Soa3 mpciv_if_active(dsl_handle* h) { return h->pci_active ? mpciv(h) : kNoSoa3; }

inline int n_fluid_of(const dsl_handle* h) { return h->n - h->nb; }
inline Bnd bnd_of(const dsl_handle* h) { return Bnd{h->nb > 0 ? h->ids[h->cur_ids] : nullptr, n_fluid_of(h)}; }

// ---- defined in dslsph.hip (every one launches kernels of the kernel headers, or sits next to those that do) ----
int build_grid(dsl_handle* h, bool carry_derived);
int ensure_grid(dsl_handle* h);  // the neighbour table of the current positions: built if it is not there
Neigh neigh(const dsl_handle* h);
bool use_tiled(const dsl_handle* h);
int density_pass(dsl_handle* h);
int force_integrate(dsl_handle* h, int part = 0);
int pci_begin_step(dsl_handle* h);
int pci_iterate(dsl_handle* h);
int pci_check(dsl_handle* h);
int pci_end_step(dsl_handle* h);
void update_split(dsl_handle* h);
int slab_pack_on(dsl_handle* h, hipStream_t st, float width_full, float width, bool from_output, float* dev_lo, float* dev_hi,
                 int cap_full, int cap_x);
int slab_append_shifted(dsl_handle* h, const float* dev_message_a, const float* dev_message_b, int cap_full, int cap_xonly,
                        float shift_a, float shift_b);

// ---- defined in collider_host.hip ----
void col_index_free(dsl_handle* h);
int col_index_update(dsl_handle* h, bool on, float edge_req);
// step: called by a step driver -- the rigid bodies' poses are integrated behind the pass (DSL_OPT_BODIES_INTEGRATE)
int collide_pass(dsl_handle* h, bool step = false);

// ---- defined in volume.hip ----
int volume_brick_count(dsl_handle* h, int which, double* value);  // DSL_OPT_VOLUME_LDS_BRICKS (0), _FALLBACK_BRICKS, _EMPTY_BRICKS, _STAGED_RECORDS (3)

// dsl_field_volume into vol_stage alone, with every refusal of dsl_field_volume (dsl_field_surface)
int field_volume_staged(dsl_handle* h, int scalar_buffer, const float origin[3], const float step[3], const int32_t dims[3]);

// ---- defined in surface.hip ----
int surface_option(dsl_handle* h, int option, double* value);  // DSL_OPT_SURFACE_* (get)
void surface_free(dsl_handle* h);
// ... and what surface_mesh.hip shares with it: the checked lattice of a call (nb: its bricks of 8 x 8 x 4 cubes, 0 without
// cubes); the triangle count and scan into surf_scan / surf_ctr (T also to dev_count, or NULL); the levels of a scan over n
// values and the array they take; the scan itself, one timing entry under kid; a blocking read of surf_ctr
struct SurfLattice;
int surf_lattice(dsl_handle* h, const char* who, const float* origin, const float* step, const int32_t* dims, SurfLattice* g,
                 long long* nb);
int surf_count(dsl_handle* h, const float* vol, const SurfLattice& g, long long nb, float iso, long long* dev_count);
size_t surf_scan_layout(long long n, std::vector<long long>* len, std::vector<size_t>* first);
int surf_scan_run(dsl_handle* h, int kid, unsigned long long* s, const std::vector<long long>& len, const std::vector<size_t>& first,
                  unsigned long long* total_a, long long* total_b);
int surf_read_ctr(dsl_handle* h, unsigned long long* two);

// ---- defined in surface_mesh.hip ----
int surface_mesh_option(dsl_handle* h, int option, double* value);  // DSL_OPT_SURFACE_VERTICES and the mesh phases' ms (get)
void surface_mesh_free(dsl_handle* h);

// ---- defined in sdf.hip ----
int sdf_option(dsl_handle* h, int option, double* value);  // DSL_OPT_SDF_* and DSL_OPT_COLLIDER_VOLUME (get)
void sdf_free(dsl_handle* h);
int collide_volume_pass(dsl_handle* h);  // the collide pass while a volume collider is set

// ---- defined in sdf_rigid.hip ----
void sdf_rigid_free(dsl_handle* h);
int collide_volume_rigid_reset(dsl_handle* h);  // motion off, the accumulators at zero (dsl_collider_set_volume)
int collide_volume_rigid_pass(dsl_handle* h);   // the collide pass while a motion is set: the rigid pass and the fold
int collide_volume_rigid_query(dsl_handle* h, float* qd, float* qn);  // dsl_collider_volume_query's launch at the pose in force

// ---- defined in bodies.hip ----
void bodies_free(dsl_handle* h);
int bodies_pass(dsl_handle* h, bool integrate);  // the collide pass while bodies exist: the pass, the fold, the integration

// ---- defined in contact.hip ----
void contact_release(dsl_handle* h);       // the lists, the tables and the partial sums go, and leave DSL_OPT_DEVICE_BYTES
int contact_lists(dsl_handle* h);          // the contact points of every body that has none yet (blocking)
int contact_list_of(dsl_handle* h, int b); // the contact points of the body dsl_body_add is about to publish as b (blocking)
int contact_step(dsl_handle* h);           // a step driver's detect, table fold and solve for DSL_OPT_BODIES_CONTACT
int contact_option_set(dsl_handle* h, double value);
int contact_option_get(dsl_handle* h, int option, double* value);

// ---- defined in sources.hip ----
void sources_free(dsl_handle* h);
// a step driver's sinks and emitters of the step about to run, in front of its neighbour build; nothing while none exists
int sources_step(dsl_handle* h);
int sources_option_set(dsl_handle* h, double value);                // DSL_OPT_SINK_EVERY
int sources_option_get(dsl_handle* h, int option, double* value);  // DSL_OPT_EMITTERS .. DSL_OPT_SINK_EVERY

// ---- defined in record.hip ----
void record_free(dsl_handle* h);
int record_frame_due(dsl_handle* h);  // the frame of the step about to run, if the schedule asks for one
// a step driver's hook, ahead of everything of the step (its sinks and emitters included); nothing while no recorder is set
inline int record_step(dsl_handle* h) { return h->rec ? record_frame_due(h) : DSL_OK; }
int record_option_get(dsl_handle* h, int option, double* value);  // DSL_OPT_RECORD_FRAMES .. DSL_OPT_RECORD_COPY_MS
int record_sync(dsl_handle* h);  // dsl_sync's share: waits for the copy stream; nothing while no recorder is set

}  // namespace dsl
