// volume.hip -- field volumes: SPHField.Interpolate (sph_field.go:124-135) at every point of a regular lattice
// (grid.Grid.GridPosition, geom/grid/point-grid.go:59-63), evaluated and left on the device (dsl_field_volume).  A
// translation unit of its own with its two kernels and their host side; its kernel list is
// tests/golden/device_kernels_volume.txt.  Same flags as dslsph.hip: -ffp-contract=off keeps the voxel coordinate
// origin + step * idx at two roundings in both math modes.
//
//   k_volume_sweep   one lane per voxel, the candidate sweep over global memory: k_field_interpolate's loop body
//                    (kernels_sph.hpp), so the same bits at the same points.  DSL_MATH_EXACT, DSL_NEIGH_LSH_REF,
//                    DSL_OPT_VOLUME_BRICKS = 0, and the voxels of a brick whose image does not fit.
//   k_volume_bricks  DSL_MATH_FAST, grid neighbours: a workgroup owns a brick of 8 x 8 x 4 voxels, stages the particles of
//                    the cells within one cell of the brick's own cells into LDS once -- (x, y, z, m/rho_j) and f_j, 20
//                    bytes, the cells' cell-start values alongside -- and every voxel walks its own 27 cells (9 x-runs)
//                    inside that image, in the sweep's order with the sweep's arithmetic.  No atomics in the sums.
#include "engine.hpp"
#include "sph_device.hpp"

namespace dsl {

constexpr int kVolBlock = 256;
// a brick: 2 x 2 x 1 waves of 4 x 4 x 4 voxels each, so that the lanes of a wave are voxels of the same or of adjacent
// cells and their trip counts agree (at step = h / 2 a wave covers 2 x 2 x 2 cells)
constexpr int kVolBX = 8, kVolBY = 8, kVolBZ = 4;
// The LDS image: 2048 records (32 KiB + 8 KiB), 1024 cell-start values, 64 row offsets per wave -- 45 KiB, three workgroups per CU.  At
// step = h / 2 a brick reaches 6 x 6 x 4 cells: 24 rows, 168 cell-start values, 1152 records at 8 particles per cell.
constexpr int kVolCap = 2048;
constexpr int kVolMaxStarts = 1024;
constexpr int kVolMaxRows = kWave;  // (the rows' prefix is one wave scan)
constexpr int kVolCounters = 4;

namespace {
// k_field_interpolate's sum at (x, y, z), candidates from global memory
template <bool FAST>
__device__ __forceinline__ float vol_sum_global(const DevConsts& c, const Neigh& nb, const CSoa3& p,
                                                const float* __restrict__ rho, int field, float xi, float yi, float zi) {
  float sum = 0.f;
  for_each_candidate(c, nb, xi, yi, zi, [&](int j) {
    const float dx = xi - p.x[j], dy = yi - p.y[j], dz = zi - p.z[j];
    const float dist = dsl_sqrt<FAST>(dist2<FAST>(dx, dy, dz));
    if (!in_support(c, nb, dist)) return;
    const float weight = dsl_div<FAST>(c.mass, rho[j]) * kern_F<FAST>(c, dist);
    const float u = weight * scalar_field<FAST>(c, field, rho, j);
    sum += u;
  });
  return sum;
}
}  // namespace

template <bool FAST>
__global__ __launch_bounds__(kVolBlock) void k_volume_sweep(DevConsts c, Neigh nb, CSoa3 p, const float* __restrict__ rho,
                                                            int field, Lattice g, int nvox, float* __restrict__ out) {
  const int v = blockIdx.x * kVolBlock + threadIdx.x;  // (at most 2^30 voxels)
  if (v >= nvox) return;
  const int i = v % g.n[0], jk = v / g.n[0];
  const int j = jk % g.n[1], k = jk / g.n[1];
  out[v] = vol_sum_global<FAST>(c, nb, p, rho, field, lattice_coord(g.o[0], g.s[0], i), lattice_coord(g.o[1], g.s[1], j),
                                lattice_coord(g.o[2], g.s[2], k));
}

// A lane's voxel in brick b: bricks x fastest; inside a brick 2 x 2 x 1 waves of 4 x 4 x 4 lanes (CUBES = true: the LDS
// walk, whose trip counts agree inside a cell) or lanes x fastest, a wave an 8 x 8 plane (the global sweep, whose loads
// coalesce along x: consecutive lanes walk overlapping slot ranges)
struct VolVoxel {
  int bi, bj, bk;
  bool mine;  // inside the lattice (the bricks of the upper faces overhang)
  float x, y, z;
  size_t at;
};
template <bool CUBES>
__device__ __forceinline__ VolVoxel vol_voxel(const Lattice& g, int b, int nbx, int nby, int tid) {
  const int lane = tid & (kWave - 1), wave = tid / kWave;
  VolVoxel v;
  v.bi = b % nbx;
  const int bjk = b / nbx;
  v.bj = bjk % nby;
  v.bk = bjk / nby;
  const int vi = v.bi * kVolBX + (CUBES ? (wave & 1) * 4 + (lane & 3) : lane & 7);
  const int vj = v.bj * kVolBY + (CUBES ? (wave >> 1) * 4 + ((lane >> 2) & 3) : lane >> 3);
  const int vk = v.bk * kVolBZ + (CUBES ? lane >> 4 : wave);
  v.mine = vi < g.n[0] && vj < g.n[1] && vk < g.n[2];
  v.x = lattice_coord(g.o[0], g.s[0], vi);
  v.y = lattice_coord(g.o[1], g.s[1], vj);
  v.z = lattice_coord(g.o[2], g.s[2], vk);
  v.at = ((size_t)vk * g.n[1] + vj) * g.n[0] + vi;
  return v;
}

// ctr[0] bricks swept out of LDS, [1] bricks whose image did not fit (global sweep), [2] bricks with no particle in reach,
// [3] records the LDS bricks staged
__global__ __launch_bounds__(kVolBlock) void k_volume_bricks(DevConsts c, const int* __restrict__ cell_start, CSoa3 p,
                                                             const float* __restrict__ rho, int field, Lattice g,
                                                             int nbx, int nby, float* __restrict__ out,
                                                             unsigned long long* __restrict__ ctr) {
  __shared__ float4 s_rec[kVolCap];
  __shared__ float s_f[kVolCap];
  __shared__ int s_start[kVolMaxStarts];
  __shared__ int s_base[kVolBlock / kWave][kVolMaxRows];  // (every wave keeps the rows' prefix for itself: no barrier for it)

  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int b = blockIdx.x;
  const VolVoxel v = vol_voxel<true>(g, b, nbx, nby, tid);
  const int bi = v.bi, bj = v.bj, bk = v.bk;
  const bool mine = v.mine;
  const float xi = v.x, yi = v.y, zi = v.z;
  const size_t at = v.at;

  // The cells of the brick's voxels: coordinate and cell rule are both monotone, so per axis they lie between the first
  // and the last voxel's cell; one more cell on every side (clamped) holds everything within h of them.
  int lo[3], hi[3];
  const int first[3] = {bi * kVolBX, bj * kVolBY, bk * kVolBZ};
  const int edge[3] = {kVolBX, kVolBY, kVolBZ};
  for (int a = 0; a < 3; ++a) {
    const int last = min(first[a] + edge[a], g.n[a]) - 1;
    const int c0 = cell_coord(lattice_coord(g.o[a], g.s[a], first[a]), c.gmin[a], c.inv_cell, c.dims[a]);
    const int c1 = cell_coord(lattice_coord(g.o[a], g.s[a], last), c.gmin[a], c.inv_cell, c.dims[a]);
    lo[a] = max(c0 - 1, 0);
    hi[a] = min(c1 + 1, c.dims[a] - 1);
  }
  const int ncx = hi[0] - lo[0] + 1, ncy = hi[1] - lo[1] + 1, ncz = hi[2] - lo[2] + 1;
  const int nrows = ncy * ncz, row_len = ncx + 1, nstarts = nrows * row_len;

  bool fits = nrows <= kVolMaxRows && nstarts <= kVolMaxStarts;  // (uniform: every operand is)
  int total = 0;
  if (fits) {
    // the cell-start values of the brick's cells, row by row: row_len of them, the end of the row's last cell included
    for (int e = tid; e < nstarts; e += kVolBlock) {
      const int r = e / row_len, xo = e - r * row_len;
      const int ry = r % ncy, rz = r / ncy;
      s_start[e] = cell_start[((lo[2] + rz) * c.dims[1] + (lo[1] + ry)) * c.dims[0] + lo[0] + xo];
    }
    lds_barrier();
    // where each row's records begin in the image: an exclusive prefix over the rows' lengths, one scan in every wave
    const int len = lane < nrows ? s_start[lane * row_len + ncx] - s_start[lane * row_len] : 0;
    int incl = len;
    for (int off = 1; off < kWave; off <<= 1) {
      const int o = __shfl_up(incl, off, kWave);
      if (lane >= off) incl += o;
    }
    s_base[wave][lane] = incl - len;
    total = __shfl(incl, kWave - 1, kWave);
    fits = total <= kVolCap;
  }

  if (!fits) {  // the image does not fit: this brick's voxels take the global sweep, dealt to the lanes anew
    if (tid == 0) atomicAdd(&ctr[1], 1ull);
    const VolVoxel w = vol_voxel<false>(g, b, nbx, nby, tid);
    if (w.mine) out[w.at] = vol_sum_global<true>(c, grid_neigh(cell_start), p, rho, field, w.x, w.y, w.z);
    return;
  }
  if (total == 0) {  // no particle in reach: zeros, nothing to stage
    if (tid == 0) atomicAdd(&ctr[2], 1ull);
    if (mine) out[at] = 0.f;
    return;
  }
  if (tid == 0) {
    atomicAdd(&ctr[0], 1ull);
    atomicAdd(&ctr[3], (unsigned long long)total);
  }

  // stage: a row is one contiguous slot range; the waves take the rows in turn
  for (int r = wave; r < nrows; r += kVolBlock / kWave) {
    const int j0 = s_start[r * row_len], len = s_start[r * row_len + ncx] - j0, base = s_base[wave][r];
    for (int q = lane; q < len; q += kWave) {
      const int j = j0 + q;
      s_rec[base + q] = make_float4(p.x[j], p.y[j], p.z[j], dsl_div<true>(c.mass, rho[j]));
      s_f[base + q] = scalar_field<true>(c, field, rho, j);
    }
  }
  lds_barrier();
  if (!mine) return;

  // the voxel's own 27 cells as 9 x-runs, z, y, then slots ascending: for_each_grid_candidate's order.  (The bounds are
  // the image's; they are the grid's whenever the grid's are tighter.)
  const int cx = cell_coord(xi, c.gmin[0], c.inv_cell, c.dims[0]);
  const int cy = cell_coord(yi, c.gmin[1], c.inv_cell, c.dims[1]);
  const int cz = cell_coord(zi, c.gmin[2], c.inv_cell, c.dims[2]);
  const int x0 = min(max(cx - 1, lo[0]), hi[0]) - lo[0], x1 = max(min(cx + 1, hi[0]), lo[0]) - lo[0];
  float sum = 0.f;
  for (int dz = -1; dz <= 1; ++dz) {
    const int zz = cz + dz;
    if (zz < lo[2] || zz > hi[2]) continue;
    for (int dy = -1; dy <= 1; ++dy) {
      const int yy = cy + dy;
      if (yy < lo[1] || yy > hi[1]) continue;
      const int r = (zz - lo[2]) * ncy + (yy - lo[1]);
      const int shift = s_base[wave][r] - s_start[r * row_len];
      const int qb = s_start[r * row_len + x0] + shift, qe = s_start[r * row_len + x1 + 1] + shift;
      for (int q = qb; q < qe; ++q) {
        const float4 rec = s_rec[q];
        const float dx = xi - rec.x, dy2 = yi - rec.y, dz2 = zi - rec.z;
        const float dist = dsl_sqrt<true>(dist2<true>(dx, dy2, dz2));
        if (!(dist < c.h)) continue;
        const float weight = rec.w * kern_F<true>(c, dist);
        const float u = weight * s_f[q];
        sum += u;
      }
    }
  }
  out[at] = sum;
}

int volume_brick_count(dsl_handle* h, int which, double* value) {
  unsigned long long ctr[4] = {0, 0, 0, 0};
  if (h->vol_last_bricks) {
    HIP_TRY(h, hipMemcpyAsync(ctr, h->vol_ctr, sizeof(ctr), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
  }
  *value = (double)ctr[which];
  return DSL_OK;
}

}  // namespace dsl

using namespace dsl;

namespace {
// dsl_field_volume; to_stage: into the library's staging array, which is then the only output (dsl_field_surface)
int field_volume(dsl_handle* h, int scalar_buffer, const float origin[3], const float step[3], const int32_t dims[3],
                 float* dev_out, float* host_out, bool to_stage) {
  // every refusal comes before anything is touched, the skin episode included
  if (h->c.n_ptr || h->c.slab_axis >= 0) return fail(h, DSL_ERR_UNSUPPORTED, "field operators are not available in slab mode");
  const int field = scalar_buffer == DSL_BUF_DENSITIES ? 0 : (scalar_buffer == DSL_BUF_PRESSURES ? 1 : -1);
  if (field < 0) return fail(h, DSL_ERR_INVALID, "dsl_field_volume: scalar_buffer must be DSL_BUF_DENSITIES or DSL_BUF_PRESSURES");
  Lattice g;
  long long nvox = 0;
  if (int rc = lattice_check(h, "dsl_field_volume", origin, step, dims, 1, &g, &nvox)) return rc;
  if (!dev_out && !host_out && !to_stage) return fail(h, DSL_ERR_INVALID, "dsl_field_volume: dev_out and host_out are both NULL");
  if (h->skin_live)
    if (int rc = skin_settle(h)) return rc;
  if (int rc = ensure_grid(h)) return rc;

  float* out = dev_out;
  if (!out) {
    if (int rc = reserve(h, h->vol_stage, (size_t)nvox, "dsl_field_volume: the staging array")) return rc;
    out = h->vol_stage.p;
  }

  const bool fast = h->prm.math_mode == DSL_MATH_FAST;
  const bool bricks = h->vol_bricks && fast && !h->lsh;
  const CSoa3 p = cpos(h);
  h->vol_last_bricks = bricks;
  int rc = DSL_OK;
  if (bricks) {
    const int nbx = (g.n[0] + kVolBX - 1) / kVolBX, nby = (g.n[1] + kVolBY - 1) / kVolBY, nbz = (g.n[2] + kVolBZ - 1) / kVolBZ;
    // (at most 2^30 voxels, and a brick holds at least 4 of them whatever the shape: at most 2^28 workgroups)
    const long long nb = (long long)nbx * nby * nbz;
    HIP_TRY(h, hipMemsetAsync(h->vol_ctr, 0, kVolCounters * sizeof(unsigned long long), h->stream));
    rc = timed(h, DSL_K_VOLUME, [&] {
      hipLaunchKernelGGL(k_volume_bricks, dim3((unsigned)nb), dim3(kVolBlock), 0, h->stream, h->c, h->cell_start, p, h->rho, field,
                         g, nbx, nby, out, h->vol_ctr);
    });
  } else {
    const dim3 grid((unsigned)((nvox + kVolBlock - 1) / kVolBlock)), block(kVolBlock);
    rc = timed(h, DSL_K_VOLUME, [&] {
      if (fast) hipLaunchKernelGGL(k_volume_sweep<true>, grid, block, 0, h->stream, h->c, neigh(h), p, h->rho, field, g, (int)nvox, out);
      else hipLaunchKernelGGL(k_volume_sweep<false>, grid, block, 0, h->stream, h->c, neigh(h), p, h->rho, field, g, (int)nvox, out);
    });
  }
  if (rc) return rc;
  if (host_out) {
    HIP_TRY(h, hipMemcpyAsync(host_out, out, (size_t)nvox * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
  }
  return DSL_OK;
}
}  // namespace

namespace dsl {
int field_volume_staged(dsl_handle* h, int scalar_buffer, const float origin[3], const float step[3], const int32_t dims[3]) {
  return field_volume(h, scalar_buffer, origin, step, dims, nullptr, nullptr, true);
}
}  // namespace dsl

int dsl_field_volume(dsl_handle* h, int scalar_buffer, const float origin[3], const float step[3], const int32_t dims[3],
                     float* dev_out, float* host_out) {
  CHECK_HANDLE_ONLY(h);
  return field_volume(h, scalar_buffer, origin, step, dims, dev_out, host_out, false);
}
