/*
 * dslsph.h -- C ABI of libdslsph.so, the MI355X (gfx950) SPH particle-step engine that
 * sits where dieselfluid's OpenCL path sits (compute/gpu + solver/pcisph GPU driver).
 *
 * Plain C: opaque handle, plain pointers and sizes, int status codes.  No torch types,
 * no C++ types.  Bound from Go through cgo (bindings/go/dslsph), from C++ through
 * dieselfluid_amd/host/dieselfluid.hpp and from Python through ctypes
 * (dieselfluid_amd/_lib.py).  See INTEGRATION.md for the reference-side stubs.
 *
 * Every entry point cites the reference interface it replaces
 * (file:line relative to the dieselfluid repository root).
 *
 * Threading: a handle is single-owner (not thread-safe); every call re-selects the
 * handle's device first because goroutines migrate between OS threads.  Host pointers
 * are never retained after a call returns (cgo pointer rule).
 */
#ifndef DSLSPH_H
#define DSLSPH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSL_ABI_VERSION 1

/* status codes: 0 = ok; negative = error, text from dsl_last_error() */
enum {
  DSL_OK = 0,
  DSL_ERR_INVALID = -1,  /* bad argument / bad state            */
  DSL_ERR_DEVICE = -2,   /* HIP runtime error                   */
  DSL_ERR_NOMEM = -3,    /* host or device allocation failure   */
  DSL_ERR_UNSUPPORTED = -4,
  DSL_ERR_OVERFLOW = -5  /* slab exchange: a band message, the particle capacity or the split margin was outgrown */
};

/* Named device buffers; the names are the ones the reference registers in
 * solver/pcisph/pcisph_gpu_darwin.go:67-76 ("positions", "velocities", "forces",
 * "densities", "pressures", "temps").  Host layout is the reference's: xyz interleaved
 * float32 (model/particle_array.go:5-15); the library converts to SoA on device. */
enum {
  DSL_BUF_POSITIONS = 0,  /* N*3 floats */
  DSL_BUF_VELOCITIES = 1, /* N*3 floats */
  DSL_BUF_FORCES = 2,     /* N*3 floats */
  DSL_BUF_DENSITIES = 3,  /* N floats   */
  DSL_BUF_PRESSURES = 4,  /* N floats   */
  DSL_BUF_PCI_POSITIONS = 5,  /* "temps".pos, N*3: predictor state of pcisph_darwin.go:28-41 */
  DSL_BUF_PCI_VELOCITIES = 6, /* "temps".vel, N*3 */
  DSL_BUF_COUNT = 7
};

enum {
  DSL_NEIGH_LSH_REF = 0, /* the reference's sampler: 8-bit random-projection LSH, 255 buckets, 100
                            samples with duplicates (sampler/lsh/lsh.go); parity mode, EXACT math only */
  DSL_NEIGH_GRID = 1     /* all j with |xi-xj| < h via uniform-grid counting sort */
};
enum {
  DSL_MATH_EXACT = 0, /* IEEE float32, one rounding per reference operation, f64 pow */
  DSL_MATH_FAST = 1   /* fused multiply-add, hardware rcp/rsq, float32 pow          */
};

/* Parameter block.  The first nine fields are the reference's "sizes" and "floats"
 * blocks (pcisph_gpu_darwin.go:60-61); the rest are the reference's compile-time
 * constants made explicit.  dsl_params_reference() fills in the reference's values. */
typedef struct dsl_params {
  uint32_t struct_size; /* = sizeof(dsl_params); ABI check */
  uint32_t abi_version; /* = DSL_ABI_VERSION               */
  /* "sizes" */
  int32_t n_particles;     /* field.Particles.N()                   */
  int32_t n_boundary;      /* Total()-N() (0 in sph.Init: fluid.go:70) */
  int32_t lsh_buckets;     /* carried for the Go side; unused here  */
  int32_t lsh_bucket_size; /* carried for the Go side; unused here  */
  /* "floats" */
  float dt;      /* SPH.CFL()   model/sph/fluid.go:111-114 (0.01) */
  float mass;    /* field.Mass()                         (1.0)    */
  float delta;   /* SPH.Delta() fluid.go:204,221-273              */
  float max_vel; /* SPH.MaxV()  initial value                     */
  float h;       /* kernel length fluid.go:48            (1.0)    */
  /* constants of the reference */
  float ref_density; /* ParticleArray.D0() particle_array.go:26 (N/8)  */
  float mu;          /* VISCOSITY_WATER fluid.go:18 (1.3059)           */
  float eos_w;       /* model/model.go:94 (2.15)                       */
  float eos_gamma;   /* model/model.go:93 (7.16)                       */
  float eos_d0_grad; /* FLUID_DENSITY, field_types.go:41 (87.0)        */
  float pressure_sign;       /* +1: fluid.go:168-169 adds the gradient  */
  int32_t visc_running_mass; /* 1: sph_field.go:265 running-sum * m     */
  float force_reset[3];      /* fluid.go:193 (0,-9.81*m,0)              */
  float external[3];         /* wcsph.go:19  (0,-9.81,0)                */
  int32_t wcsph_pressure_force; /* 0: absent from wcsph.go:14-26        */
  int32_t wcsph_viscosity;      /* 0: absent from wcsph.go:14-26        */
  int32_t pci_max_iters;        /* pcisph_darwin.go:49 (5)              */
  float pci_max_error;          /* pcisph_darwin.go:50 (0.01)           */
  /* build-defined: axis-aligned wall box applied at the end of Update */
  int32_t walls;
  float box_min[3], box_max[3];
  float restitution;
  /* uniform grid for the neighbour table; cell edge = h */
  float grid_min[3], grid_max[3];
  int32_t neigh_mode; /* DSL_NEIGH_GRID */
  int32_t math_mode;  /* DSL_MATH_*     */
  int32_t capacity;   /* particle slots to allocate (>= n_particles); 0 = n_particles.
                         Slab ranks need room for migrants and ghosts. */
  /* build-defined terms of BASELINE configs[4] (no reference counterpart), 0 = off:
   *   xsph_eps: positions advect with v + eps * sum_j (m/rho_j) (v_j - v_i) F(r_ij)
   *   st_kappa: cohesion force F_i += kappa * sum_j m (x_j - x_i) F(r_ij)          */
  float xsph_eps, st_kappa;
  /* 0 (default): slots inside a grid cell are ascending in particle id after every neighbour build, so
   * every neighbour sum runs in a fixed order and results are reproducible bit for bit from run to run
   * (and, in DSL_MATH_EXACT, equal to the reference's sums taken cell by cell).  1: keep the order the
   * counting sort's atomics produce (saves the ordering pass of the scatter; last-bit differences between runs).
   * Ignored -- the cells stay ordered -- while visc_running_mass = 1 and mass != 1: that viscosity (sph_field.go:265)
   * multiplies its running sum by m after every neighbour, so the in-cell order would decide the viscous force of
   * WCSPH, ViscousAll and PCISPH, not only its last bit. */
  int32_t sort_unordered;
  /* reserved[0]: budget, in MiB, for each of the two side arrays that cost memory per GRID CELL rather than per particle
   * (the cells' key rows of the one-pass in-cell ordering: 128 B per cell; the PCISPH query rows: 512 B per cell); 0 = the
   * larger of 4 GiB and 64 B per particle slot.  An array beyond its budget is not allocated and the kernels take the
   * forms that need none (two-pass ordering, the queries' sorted array): same results, a few per cent slower.
   * reserved[1..3]: 0. */
  int32_t reserved[4];
} dsl_params;

/* Counters the reference keeps on the host (fluid.go:25-26,186-191) plus the PCISPH loop
 * outcome (pcisph_darwin.go:46-98). */
typedef struct dsl_stats {
  float max_vel, max_f;
  float pci_max_error;
  int32_t pci_iters;
  int64_t steps;
  int32_t grid_dims[3];
  int32_t grid_cells;
  int32_t max_cell_count; /* most crowded cell at the last neighbour build */
} dsl_stats;

/* kernel ids for dsl_timing_get */
enum {
  DSL_K_CELL_RANK = 0,
  DSL_K_SCAN = 1,
  DSL_K_SCATTER = 2,
  DSL_K_DENSITY = 3,
  DSL_K_FORCE_INTEGRATE = 4, /* fused WCSPH pressure+viscosity+external+Update */
  DSL_K_PRESSURE = 5,
  DSL_K_VISCOUS = 6,
  DSL_K_GRADIENT = 7,
  DSL_K_EXTERNAL = 8,
  DSL_K_UPDATE = 9,
  DSL_K_PCI_PREDICT = 10,
  DSL_K_PCI_DENSITY = 11,
  DSL_K_TILE_LIST = 12, /* non-empty 4x4x4-cell tiles for the LDS-tiled kernels */
  DSL_K_NEIGH_LISTS = 13, /* skin step: wide candidate sweep + neighbour lists (rebuild steps only) */
  DSL_K_COLLIDE = 14,     /* triangle-mesh collider: query + response (only while a mesh is set) */
  DSL_K_VOLUME = 15,      /* dsl_field_volume: the lattice sweep, either form */
  DSL_K_SURFACE = 16,     /* dsl_surface_extract: its count, scan and emit launches, one entry each */
  DSL_K_SURFACE_MESH = 17, /* dsl_surface_extract_indexed: its vertex count, vertex scan, vertex emit and index emit */
  DSL_K_SDF = 18,          /* dsl_mesh_distance_volume: prep, brick count, scan, brick fill, distance, sweep, sign, one entry each */
  DSL_K_COUNT = 19,        /* the ids above: the step's and the scene's kernels */
  DSL_K_SOURCES = 19,      /* sources and sinks: the emit launch, the sink count, the compaction's launches, one entry each */
  DSL_K_END = 20           /* one past the last id: dsl_timing_get takes 0 .. DSL_K_END - 1 */
};

typedef struct dsl_handle dsl_handle;

/* sph.Init's constants for an n3^3 system (model/sph/fluid.go:41-88). */
int dsl_params_reference(dsl_params *out, int n3);

/* gpu.InitOpenCL + gpu.New_ComputeGPU + New_GPUPredictorCorrector's ten RegisterBuffer
 * calls (compute/gpu/gpu.go:45-119,314; pcisph_gpu_darwin.go:36-76).  `device` is the
 * HIP device ordinal. */
int dsl_create(const dsl_params *params, int device, dsl_handle **out);
int dsl_destroy(dsl_handle *h);

/* Scalars may change between steps (dt, delta, mu, ...); n_particles and the grid box
 * may not. */
int dsl_set_params(dsl_handle *h, const dsl_params *params);
int dsl_get_params(dsl_handle *h, dsl_params *out);

/* ComputeGPU.PassFloatBuffer / ReadFloatBuffer (compute/gpu/gpu.go:343-352,332-341) and
 * the per-step EnqueueReadBufferFloat32 of pcisph_gpu_darwin.go:276-277.  Blocking;
 * `count` is the number of floats and must match the buffer. */
int dsl_upload(dsl_handle *h, int buffer, const float *host, size_t count);
int dsl_download(dsl_handle *h, int buffer, float *host, size_t count);

/* ParticleArray.AddBoundaryParticles (model/particle_array.go:123-128; fed by SPHField.BoundaryParticles,
 * model/field/sph_field.go:75-85, from Mesh.GenerateBoundaryParticles, geom/mesh/mesh.go:60-76):
 * appends count/3 position-only particles behind the current ones; needs room in
 * dsl_params.capacity.  dsl_params.n_boundary > 0 at creation is the same as NewParticleArray(n, nb, ..):
 * nb zero-filled boundary slots.  With boundary particles DSL_BUF_POSITIONS holds Total() = N + Nb
 * particles (fluid first), every other buffer N.
 * Semantics are the reference's, quirks included (oracle/dsl_oracle.c restates them first):
 *   - boundary particles are candidates of every neighbour sum with Get()'s values: position, density
 *     0, press 0, velocity 0 (particle_array.go:94-117); Density/DensityF simply count them
 *     (sph_field.go:143,163), Gradient and LaplacianForce divide by their density 0 without a guard
 *     (sph_field.go:183,259): a fluid particle with a boundary neighbour gets NaN / Inf there;
 *   - Get(N()) -- the FIRST boundary particle -- is the zero particle: it takes part in every sum at the
 *     origin, while the positions slice keeps (and dsl_download returns) what was uploaded;
 *   - no pass writes a boundary particle; Update does not move it.
 * Not available in slab mode or after dsl_set_ids. */
int dsl_add_boundary_particles(dsl_handle *h, const float *host_positions, size_t count);

/* Render hand-off without the per-step full read-back of pcisph_gpu_darwin.go:276-277
 * (SURVEY 8f rank 1):
 * dsl_download_decimated: every stride-th particle (host index 0, stride, 2*stride, ...) of a
 *   3-component buffer, count = 3*ceil(N/stride) floats; blocking.
 * dsl_device_pointers: the live device arrays themselves (SoA, cell-sorted slot order) for a
 *   consumer that can read device memory (another HIP kernel, graphics interop):
 *   xyz[3] component pointers of `buffer`, ids = slot -> particle index, n = slot count.
 *   Valid until the next call that steps, uploads or rebuilds the neighbour table. */
int dsl_download_decimated(dsl_handle *h, int buffer, int stride, float *host, size_t count);
int dsl_device_pointers(dsl_handle *h, int buffer, const float **xyz, const int32_t **ids, int *n);

/* lsh.Allocate's random projection vectors (sampler/lsh/lsh.go:32-40): hash_bits x 3 floats.
 * The reference draws them from math/rand seeded with the wall-clock second; here they are an
 * explicit input.  DSL_NEIGH_LSH_REF only. */
int dsl_set_hash_vectors(dsl_handle *h, const float *vectors, int hash_bits);
/* HashSampler.GetData1D (lsh.go:70-80): the flattened buckets x lsh_bucket_size table */
int dsl_lsh_download_table(dsl_handle *h, int32_t *out, size_t count);

/* SPH.NN() / HashSampler.UpdateSampler (fluid.go:100-102, sampler/lsh/lsh.go:126-133):
 * rebuilds the neighbour table (cell hash, histogram, prefix sum, counting-sort scatter). */
int dsl_build_neighbours(dsl_handle *h);

/* The whole-array passes of model/sph/fluid.go, one to one. */
int dsl_density_pass(dsl_handle *h);                  /* DensityAll            :127-131 */
int dsl_pressure_pass(dsl_handle *h);                 /* PressureAll           :134-142 */
int dsl_viscous_pass(dsl_handle *h);                  /* ViscousAll            :146-152 */
int dsl_external_pass(dsl_handle *h, const float f[3]); /* ExternalAll         :155-161 */
int dsl_gradient_pressure_pass(dsl_handle *h);        /* GradientPressureForce :164-172 */
int dsl_update_pass(dsl_handle *h);                   /* Update                :175-197 */
/* Fused form of [GradientPressureForce][ViscousAll] ExternalAll PressureAll Update used by
 * dsl_wcsph_step; needs densities from dsl_density_pass. */
int dsl_force_pass(dsl_handle *h);

/* The SPHField operators no solver calls (model/field/sph_field.go), evaluated on the current
 * state (densities as left by the last dsl_density_pass).  tensor_buffer is
 * DSL_BUF_VELOCITIES or DSL_BUF_FORCES; scalar_buffer is DSL_BUF_DENSITIES (DensityField) or
 * DSL_BUF_PRESSURES (PressureField.Value = TaitEos(rho, 87.0, 0), field_types.go:39-42).
 * Results come back in host order; blocking. */
int dsl_field_divergence(dsl_handle *h, int tensor_buffer, float *host_out, size_t count);   /* Div         :203-227, N   */
int dsl_field_curl(dsl_handle *h, int tensor_buffer, float *host_out, size_t count);         /* Curl        :272-294, 3N  */
int dsl_field_laplacian(dsl_handle *h, int scalar_buffer, float *host_out, size_t count);    /* Laplacian   :230-248, N   */
int dsl_field_interpolate(dsl_handle *h, int scalar_buffer, const float *host_positions,     /* Interpolate :124-135      */
                          size_t n_positions, float *host_out);

/* Field volumes: SPHField.Interpolate (sph_field.go:124-135) at every point of a regular lattice (grid.Grid.GridPosition,
 * geom/grid/point-grid.go:59-63), evaluated and left on the device.
 *
 * Voxel (i, j, k) lies at origin[a] + step[a] * (float)idx[a] per axis: float32, one multiplication and one addition, each
 * rounded, never fused, in both math modes -- a caller reproduces every coordinate bit for bit.  The value is
 * dsl_field_interpolate's at that point: the same sum, arithmetic and candidate order, the same scalar_buffer
 * (DSL_BUF_DENSITIES or DSL_BUF_PRESSURES), the same treatment of boundary particles (a division by their density 0
 * included) and of DSL_NEIGH_LSH_REF, on the current state (densities as left by the last dsl_density_pass).
 *
 * The output is dims[0] * dims[1] * dims[2] floats, x fastest: voxel (i, j, k) at (k * dims[1] + j) * dims[0] + i.  This is a
 * deliberate departure from the reference's Grid.Index (point-grid.go:53-57), which is only right for cubes.
 * dev_out is device memory: written asynchronously on the handle's stream, never read by the library.  host_out is a
 * blocking copy.  Either may be NULL, not both; with host_out alone the library stages in an array of its own, allocated
 * on first use, grown on demand, counted in DSL_OPT_DEVICE_BYTES and freed by dsl_destroy (DSL_ERR_NOMEM if it cannot be
 * had: the handle stays usable).
 *
 * DSL_ERR_INVALID (dsl_last_error names the argument): a scalar_buffer other than the two, a dims entry < 1, more than
 * 2^30 voxels, a step entry that is not finite and > 0, a non-finite origin, both outputs NULL.  DSL_ERR_UNSUPPORTED in
 * slab mode, as for the field operators.  A refused call changes nothing.
 *
 * Like every entry point but the step drivers, the call first settles a live skin episode (DSL_OPT_SKIN): the next step
 * sorts and rebuilds its lists.  Two kernel forms, DSL_OPT_VOLUME_BRICKS; every launch is timed under DSL_K_VOLUME. */
int dsl_field_volume(dsl_handle *h, int scalar_buffer, const float origin[3], const float step[3],
                     const int32_t dims[3], float *dev_out, float *host_out);

/* Fluid surfaces: the iso-surface of a volume on dsl_field_volume's lattice, as triangles in the reference's mesh.Mesh
 * layout (geom/mesh/mesh.go:11-14; dsl_collider_set_mesh takes the same): 9 floats of vertices per triangle, 3 of normal.
 *
 * The rule is build-defined (the reference has no extractor): marching tetrahedra.  A cube is the 8 voxels (i..i+1, j..j+1,
 * k..k+1), corner c at offset (c & 1, (c >> 1) & 1, (c >> 2) & 1); cubes are numbered x fastest.  Every cube splits into the
 * same six tetrahedra around the diagonal from corner 0 to corner 7: for the axis permutations (a, b, c) in the order xyz, xzy,
 * yxz, yzx, zxy, zyx the tetrahedron {0, e_a, e_a | e_b, 7}.  A voxel is inside when value >= iso.  A tetrahedron with one
 * vertex i alone on its side gives one triangle through the edge points P(i, j) of the other three vertices j, ascending;
 * two inside a < b and two outside c < d give the quad P(a, c), P(a, d), P(b, d), P(b, c) as (q0, q1, q2) and (q0, q2, q3).
 * Winding comes from a table (csrc/surface_table.hpp, generated by tools/make_surface_table.py): a triangle whose normal
 * would point inwards has its second and third vertex exchanged, so (b - a) x (c - a) points from inside to outside, towards
 * lower values.  An edge point lies on the edge from the voxel with the smaller linear index u to the larger w:
 * t = (iso - v_u) / (v_w - v_u), p = x_u + t * (x_w - x_u) per component with x = origin + step * idx as in dsl_field_volume:
 * float32, every operation rounded once, IEEE division, nothing fused, the same in both math modes -- every cube that
 * shares an edge computes the same bits, so the triangles join exactly.  The normal is n = (b - a) x (c - a) (differences
 * and products each rounded) divided by len = sqrt((nx^2 + ny^2) + nz^2), or (0, 0, 0) when len is not > 0.
 * A cube with a corner that is not finite emits nothing: boundary particles make NaN voxels (dsl_add_boundary_particles),
 * and the surface has a HOLE there.  A voxel that equals iso exactly makes triangles of zero area; they are kept, so the
 * count depends on the inside masks alone.  At most 12 triangles per cube.
 * Order: bricks of 8 x 8 x 4 cubes ascending (x fastest; the first brick starts at cube 0), inside a brick its cubes
 * ascending (x fastest), tetrahedra 0..5 inside a cube, table order inside a tetrahedron.  Every position comes from counts
 * and a prefix sum, none from an atomic: two runs give the same bytes.
 *
 * dsl_surface_extract reads dev_volume (dims[0] * dims[1] * dims[2] floats of device memory, x fastest) and no particle
 * state: it does not settle a live skin episode and works on slab handles too.  It writes the first min(T, cap_triangles)
 * triangles to dev_vertices (9 floats each) and, unless NULL, dev_normals (3 floats each), and nothing beyond them; T, the
 * full number of triangles whatever the capacity, goes to dev_count (device memory, unless NULL) and to host_count.
 * Asynchronous on the handle's stream unless host_count is given: that is a blocking 8-byte copy.  cap_triangles = 0 with
 * NULL outputs is the counting call.  A dims entry of 1 means no cubes: T = 0.  The library keeps 8 bytes per brick of
 * 8 x 8 x 4 cubes (and 1/255 more) of its own, grown on demand and counted in DSL_OPT_DEVICE_BYTES.  Offsets are 64-bit;
 * the voxel limit is dsl_field_volume's 2^30.
 * DSL_ERR_INVALID (dsl_last_error names the argument): dev_volume NULL, a dims entry < 1, more than 2^30 voxels, a step
 * entry that is not finite and > 0, a non-finite origin or iso, cap_triangles > 0 with dev_vertices NULL.  A refused call
 * touches nothing.
 *
 * dsl_field_surface is the end-to-end call for a host without device memory: dsl_field_volume into the library's staging
 * array, the extraction into a second array of the library's own (grown on demand, counted in DSL_OPT_DEVICE_BYTES, freed by
 * dsl_destroy), and a blocking copy of the first min(T, cap_triangles) triangles; *n_triangles = T.  Refusals and slab
 * behaviour (DSL_ERR_UNSUPPORTED) are dsl_field_volume's, plus a non-finite iso and cap_triangles > 0 with host_vertices
 * NULL; like dsl_field_volume it settles a live skin episode.
 *
 * Launches are timed under DSL_K_SURFACE.  DSL_OPT_SURFACE_TRIANGLES and DSL_OPT_SURFACE_ACTIVE_BRICKS describe the last call. */
int dsl_surface_extract(dsl_handle *h, const float *dev_volume, const float origin[3], const float step[3],
                        const int32_t dims[3], float iso, float *dev_vertices, float *dev_normals,
                        size_t cap_triangles, int64_t *dev_count, int64_t *host_count);
int dsl_field_surface(dsl_handle *h, int scalar_buffer, const float origin[3], const float step[3], const int32_t dims[3],
                      float iso, float *host_vertices, float *host_normals, size_t cap_triangles,
                      int64_t *n_triangles);

/* Fluid surfaces as an INDEXED mesh: the same surface as dsl_surface_extract's, with every vertex stored once, a normal per
 * vertex, and three int32 vertex ids per triangle -- what a renderer of indexed meshes (glTF) draws, smooth-shaded, without
 * a welding pass on the host.  Lattice, cubes, Kuhn tetrahedra, the inside test (value >= iso), the non-finite rule, the
 * triangle count T, the triangle order and the winding are exactly dsl_surface_extract's; the rule for the rest is
 * build-defined too:
 *
 * Vertices.  Every edge of the Kuhn triangulation is a translate of one of seven types: for a voxel u and d in 1..7, edge
 * (u, d) runs from u to w = u + (d & 1, (d >> 1) & 1, (d >> 2) & 1); u is the end with the smaller linear index.  A vertex
 * exists on edge (u, d) iff w is inside the lattice, exactly one of u, w is inside the surface, and at least one LIVE cube
 * holds both ends -- the cubes with corner 0 at u - s for the offsets s in 0..7 with (s & d) == 0; a cube is live when it
 * lies within the lattice and its 8 corners are finite.  That is exactly the set of edges some triangle touches: every
 * vertex is referenced, every reference has a vertex.  At a voxel that equals iso several vertices share their position
 * bits; they stay distinct vertices, so the mesh welded by id is a manifold where the soup welded by bits is not.
 * Position: dsl_surface_extract's edge point, f = (iso - v_u) / (v_w - v_u), p = x_u + f * (x_w - x_u), the same bits:
 * positions[indices[3 * t + e]] is vertex e of the soup's triangle t, bit for bit.
 * Vertex order: bricks of 8 x 8 x 4 VOXELS ascending, x fastest, the first at voxel 0 -- ceil(nx / 8) * ceil(ny / 8) *
 * ceil(nz / 4) of them, which can be one more per axis than the bricks of cubes; inside a brick its voxels ascending, x
 * fastest; inside a voxel d ascending.  Every id comes from counts and a prefix sum, none from an atomic.
 * Normal: the negated gradient of the volume at the vertex, towards lower values like the triangles' normals.  Per voxel p
 * and axis a, with x dsl_field_volume's coordinate: p - e_a is usable when it lies inside the lattice and its value is
 * finite, p + e_a likewise; both usable: g_a = (v+ - v-) / (x+ - x-); only +: (v+ - v_p) / (x+ - x_p); only -:
 * (v_p - v-) / (x_p - x-); neither: 0.  At the vertex G_a = g_a(u) + f * (g_a(w) - g_a(u)) with the position's f,
 * len = sqrt((Gx^2 + Gy^2) + Gz^2), n = (-G) / len, or (0, 0, 0) when len is not > 0.  float32, every difference, product,
 * sum and quotient rounded once, IEEE division and square root, nothing fused: the same bits in both math modes.
 * Limit: at most 2^28 voxels, so that every id (< 7 * 2^28) is a non-negative int32.
 *
 * dsl_surface_extract_indexed reads dev_volume and no particle state: it does not settle a live skin episode and works on
 * slab handles.  It writes the first min(V, cap_vertices) vertices to dev_positions (3 floats each) and, unless NULL, to
 * dev_normals (3 floats each), the first min(T, cap_triangles) index triples to dev_indices, and nothing beyond them.  V and
 * T are the full numbers whatever the capacities: dev_counts (two int64 of device memory, unless NULL) and host_counts take
 * [0] = V, [1] = T.  Asynchronous on the handle's stream unless host_counts is given (a blocking copy).  Capacities of 0 with
 * NULL outputs make the counting call.  A written triple may name a vertex >= cap_vertices: THE MESH IS COMPLETE ONLY WHEN
 * BOTH CAPACITIES SUFFICE (cap_vertices >= V and cap_triangles >= T).
 * Memory: besides dsl_surface_extract's 8 bytes per brick of cubes the library keeps one 32-bit word PER VOXEL -- as much as
 * the volume itself -- and 8 bytes per brick of voxels, all of its own, grown on demand, counted in DSL_OPT_DEVICE_BYTES
 * and freed by dsl_destroy.
 * DSL_ERR_INVALID (dsl_last_error names the argument): dsl_surface_extract's refusals (dev_volume NULL, a dims entry < 1, a
 * step entry that is not finite and > 0, a non-finite origin or iso), more than 2^28 voxels in dims, cap_vertices > 0 with
 * dev_positions NULL, cap_triangles > 0 with dev_indices NULL.  A refused call touches nothing.
 *
 * dsl_field_surface_indexed is to it what dsl_field_surface is to dsl_surface_extract: dsl_field_volume into the library's
 * staging array, count and scan, a blocking read of the counts, the emits into an array of the library's own grown to
 * min(V, cap_vertices) and min(T, cap_triangles), and blocking copies; counts[0] = V, counts[1] = T (counts may be NULL).
 * Refusals and slab behaviour (DSL_ERR_UNSUPPORTED) are dsl_field_volume's, plus a non-finite iso, more than 2^28 voxels,
 * cap_vertices > 0 with host_positions NULL and cap_triangles > 0 with host_indices NULL; it settles a live skin episode.
 *
 * The triangle count and its scan are dsl_surface_extract's own launches, timed under DSL_K_SURFACE; the vertex count, the
 * vertex scan, the vertex emit and the index emit are timed under DSL_K_SURFACE_MESH, one entry each.
 * DSL_OPT_SURFACE_VERTICES is V of the last indexed call; DSL_OPT_SURFACE_TRIANGLES its T. */
int dsl_surface_extract_indexed(dsl_handle *h, const float *dev_volume, const float origin[3], const float step[3],
                                const int32_t dims[3], float iso, float *dev_positions /* 3 per vertex */,
                                float *dev_normals /* 3 per vertex, or NULL */, size_t cap_vertices,
                                int32_t *dev_indices /* 3 per triangle */, size_t cap_triangles,
                                int64_t *dev_counts /* [0] = V, [1] = T; or NULL */, int64_t *host_counts /* likewise */);
int dsl_field_surface_indexed(dsl_handle *h, int scalar_buffer, const float origin[3], const float step[3],
                              const int32_t dims[3], float iso, float *host_positions, float *host_normals,
                              size_t cap_vertices, int32_t *host_indices, size_t cap_triangles, int64_t counts[2]);

/* Step drivers: one iteration of WCSPH.Run (solver/wcsph/wcsph.go:14-26) and of
 * PciMethod.Run (solver/pcisph/pcisph_darwin.go:43-101) per step.  Asynchronous: they
 * return once the work is queued; dsl_sync/dsl_download/dsl_get_stats wait. */
int dsl_wcsph_step(dsl_handle *h, int nsteps);
int dsl_pcisph_begin(dsl_handle *h); /* pcisph_darwin.go:28-41 predictor copies */
int dsl_pcisph_step(dsl_handle *h, int nsteps);
/* The same step in pieces, for hosts that have to look at the iteration error between the
 * correction sweep and the convergence check (pcisph_darwin.go:95-98) -- slab mode, where the
 * error is the maximum over all ranks:
 *   DSL_PCI_BEGIN_STEP  NN, DensityAll, ViscousAll, loop set-up        (:43-51)
 *   DSL_PCI_ITERATE     predict, DensityF + pressure accumulate, gradient force (:52-94); leaves
 *                       this handle's max density error in a device word
 *   DSL_PCI_CHECK       the early-out test of that word (:95-98); later ITERATEs are no-ops
 *                       once it has passed
 *   DSL_PCI_END_STEP    Update (:101)
 * dsl_pcisph_error_word copies the device word out (store = 0) or in (store = 1), device to
 * device and asynchronously; its bits order like the non-negative float they hold, so a MAX
 * all-reduce over uint32 is the global error. */
enum { DSL_PCI_BEGIN_STEP = 0, DSL_PCI_ITERATE = 1, DSL_PCI_CHECK = 2, DSL_PCI_END_STEP = 3 };
int dsl_pcisph_phase(dsl_handle *h, int phase);
int dsl_pcisph_error_word(dsl_handle *h, uint32_t *dev_word, int store);
/* DensityF's query points are the predictor's positions, and the reference never brings the predictor back to the
 * particles (pcisph_darwin.go:28-41: `_pos`, `_vel` are seeded once, advanced in every correction iteration): within
 * tens of steps they are cells, then whole tiles away from the particle they belong to.  The library then sorts the
 * QUERIES into the particles' grid cells before every DensityF sweep (same candidates, same order, same arithmetic per
 * query: DSL_MATH_EXACT results do not change by a bit).  mode 0 (default): switch when 0.2 % of the queries have left
 * their particle's 4x4x4-cell tile -- looked at every 4 steps through an asynchronous copy of the device's
 * counters that the next look reads (no stall; the decision trails the drift by 4 to 8 steps), a one-way switch until
 * the next dsl_pcisph_begin; 1: always; -1: never.  (While the handle's stream is being captured into a graph of the
 * host's the automatic look is skipped: set the mode.)  In slab mode every rank latches from ITS OWN counters: in
 * DSL_MATH_FAST the binned and un-binned sweeps sum in different orders, so a multi-rank FAST run's last bits depend on
 * the decomposition -- set the mode explicitly (the same on every rank) where that matters; DSL_MATH_EXACT does not care.
 * The slab step drivers do not look at `escaped` themselves: a host that runs PCISPH across slabs polls it.
 * dsl_pcisph_get_binning: the mode; whether the next correction iteration sorts its queries; and, slab mode (blocking
 * if asked for), whether a query point of an owned particle has drifted more than h beyond a slab plane since
 * dsl_pcisph_begin, i.e. out of what the 2h ghost band covers: from then on this rank's predicted densities -- the
 * pressure accumulator and the iteration's convergence error, nothing else reads them (pcisph_darwin.go:76-98) -- miss
 * neighbours that live on another rank.  Any of the three pointers may be NULL. */
int dsl_pcisph_set_binning(dsl_handle *h, int mode);
int dsl_pcisph_get_binning(dsl_handle *h, int *mode, int *active, int *escaped);

/* geom.Collider (geom/interfaces.go:11-16) as Mesh.Collision implements it (geom/mesh/mesh.go:41-57) through
 * Triangle.BarycentricCollision / Barycentric (geom/triangle/tri.go:37-101): the reference takes a list of colliders in
 * sph.Init (model/sph/fluid.go:28,41) and defines the query; nothing in it consumes the result.
 * A collider is T triangles in list order: vertices a,b,c (9 floats) and one normal n (3 floats) each.  The normal is
 * used as supplied -- not normalised, flipped or checked (InitMesh leaves the last one zero and throws its flip away,
 * mesh.go:24,30).  Several meshes: the host concatenates them in list order.
 * The query for a fluid particle is Mesh.Collision(P, V, dt = dsl_params.dt, r = radius): the FIRST triangle in list order
 * that collides wins; a particle with Mag(V) == 0 never collides.  The arithmetic is the reference's, float32 rounded once
 * per operation, and the SAME in DSL_MATH_EXACT and DSL_MATH_FAST (results are bit-identical between the two: a
 * collision is a classification).  Returns per particle: the triangle index (-1: none), its normal, the barycentric
 * coordinates (u,v,w), and point = P + V * (-dt), the position rewound (tri.go:70); zeros where nothing collides.
 * Response (build-defined, like the wall box): a colliding particle with k = ((a - P).n) / (n.V) >= 0 -- the plane lies
 * ahead along V -- is set back to `point` and v <- v - n * ((1 + restitution) * (v.n)); a receding one (k < 0) is left
 * alone.  Boundary particles are not queried; the PCISPH predictor state is not touched.
 * dsl_collider_set_mesh : T = 0 removes the mesh.  Blocking.  Not available in slab mode (DSL_ERR_UNSUPPORTED) unless
 *                         DSL_OPT_COLLIDE_SLAB is 1 (below).  A call refused for its arguments leaves the mesh that was
 *                         set; one that fails on the device (DSL_ERR_NOMEM, DSL_ERR_DEVICE) leaves the handle without a mesh.
 * dsl_collide_pass      : query + response for every fluid particle.  Asynchronous.  Without a mesh: nothing.
 * dsl_collider_query    : the four returns in host order, no response; any pointer may be NULL.  Blocking.  Not
 *                         available in slab mode, with or without DSL_OPT_COLLIDE_SLAB: its results are in host order,
 *                         which a rank does not have.
 * While a mesh is set the step drivers run the collide pass after Update: dsl_wcsph_step after force + integrate,
 * dsl_pcisph_step and DSL_PCI_END_STEP after Update (dsl_update_pass and dsl_force_pass stay one to one), the skin step
 * is not taken, and dsl_stats.max_vel / max_f stay what Update saw.  Without a mesh no kernel is launched and no result
 * changes by a bit.
 *
 * Slab ranks (DSL_OPT_COLLIDE_SLAB = 1; with 0, the default, a slab handle refuses a mesh and a handle with a mesh refuses
 * dsl_slab_config, both DSL_ERR_UNSUPPORTED).  The mesh is REPLICATED: every rank sets the same triangles, radius and
 * restitution.  The library cannot check that the ranks agree -- a rank sees its own handle only; ranks that disagree
 * compute different flows on the two sides of a plane.  A collision needs no neighbour (the query reads one particle
 * and the mesh), so what a rank adds is bookkeeping: dsl_collide_pass on a slab handle collides exactly the particles
 * the LAST INTEGRATE on this handle wrote, and nothing else --
 *   after dsl_force_pass, dsl_update_pass or DSL_PCI_END_STEP : every live slot whose position is not NaN.  (The
 *       integrate marked the ghosts NaN: they are never queried or counted, never widen a wave's broad-phase box and
 *       never make a wave walk the whole list.  A ghost needs no collision of its own: its owner collides it before the
 *       pack that sends it.)
 *   after dsl_force_pass_split(DSL_SPLIT_BAND)  : on the OUTPUT half of the state, where dsl_slab_pack_band reads, the
 *       slots whose cell before the step is a band layer -- the rule the band pack applies.
 *   after dsl_force_pass_split(DSL_SPLIT_INNER) : the slots of the other layers only; a band particle is already in a
 *       message and is not collided a second time.
 * The order is integrate -> collide -> pack / append / neighbour build.  DSL_ERR_INVALID (the text names that order): a
 * second collide without an integrate in between; a collide after dsl_slab_pack, dsl_slab_pack_band (for that phase),
 * dsl_slab_append*, dsl_slab_exchange or dsl_build_neighbours -- after an append the fresh ghosts are finite and would
 * be moved away from their owner's state, after a pack the message would be stale.  A particle that crossed a plane in
 * the integrate and is set back across it by the response is not a migrant: ownership is decided by the pack.
 * DSL_OPT_COLLIDE_HITS / _VISITS / _FULL_WAVES hold the sum over the launches of one step (split step: band + inner;
 * zeroed by the first pass after a neighbour build); DSL_K_COLLIDE times each launch.  dsl_stats.max_vel / max_f, the
 * PCISPH predictor state and the split step's margin test are what they are without the pass.  Boundary particles stay
 * refused in slab mode.
 * The native slab drivers run the pass directly after each integrate and before the pack that follows it, while a mesh
 * is set: unsplit integrate -> collide -> (planes move) -> exchange; split band integrate -> band collide -> band pack,
 * inner integrate -> inner collide -> append (the transfer still runs under the inner launches); PCISPH in
 * DSL_PCI_END_STEP, as on a single domain.  Without a mesh: the launches, transport calls and bits of a library that
 * has no such option. */
int dsl_collider_set_mesh(dsl_handle *h, const float *vertices /* 9*T */, const float *normals /* 3*T */,
                          size_t n_triangles, float radius, float restitution);
int dsl_collide_pass(dsl_handle *h);
int dsl_collider_query(dsl_handle *h, int32_t *tri /* N: index or -1 */, float *normal /* 3N */,
                       float *coord /* 3N */, float *point /* 3N */);

/* ---- implicit colliders: the distance volume of a triangle mesh, and collision against a distance volume (csrc/sdf.hip) ----
 * The reference names them ("SPH/Fluid Implicit Collision Techniques / SDF Processing", README.MD:35-39; colliders "for SDF
 * representation", render/mesh/collider.go:10-36) and implements neither: both rules below are BUILD-DEFINED, like the wall
 * box.  They are float32 with every operation rounded once and nothing fused, a dot product is (x*x + y*y) + z*z, divisions
 * and square roots are correctly rounded, and they are the same in DSL_MATH_EXACT and DSL_MATH_FAST.  tests/sdf_ref.py
 * restates them operation for operation.
 *
 * dsl_mesh_distance_volume: the lattice, coordinates (origin + step * (float)idx, each operation rounded once), output order
 * (x fastest) and dev_out / host_out behaviour are dsl_field_volume's: dev_out is written on the handle's stream, host_out is
 * blocking, with host_out alone the library stages in an array of its own (DSL_OPT_DEVICE_BYTES).  The call itself blocks
 * once, for the length of its brick lists; `vertices` (T triangles a, b, c, host memory) is not retained.  It reads no
 * particle state, does not settle a live skin episode and works on slab handles.
 *   Distance.  Per triangle d2 is the squared distance of the voxel p to the closest point q of the triangle, by the seven
 *   regions on d1 = ab.(p-a), d2 = ac.(p-a), d3 = ab.(p-b), d4 = ac.(p-b), d5 = ab.(p-c), d6 = ac.(p-c), the first that holds:
 *     d1 <= 0 and d2 <= 0: q = a;   d3 >= 0 and d4 <= d3: q = b;   d6 >= 0 and d5 <= d6: q = c;
 *     vc = d1 d4 - d3 d2 <= 0, d1 >= 0, d3 <= 0: q = a + ab (d1 / (d1 - d3));
 *     vb = d5 d2 - d1 d6 <= 0, d2 >= 0, d6 <= 0: q = a + ac (d2 / (d2 - d6));
 *     va = d3 d6 - d5 d4 <= 0, e1 = d4 - d3 >= 0, e2 = d5 - d6 >= 0: q = b + (c - b) (e1 / (e1 + e2));
 *     else s = (va + vb) + vc, q = (a + ab (vb / s)) + ac (vc / s);
 *   d2 = |p - q|^2.  A triangle whose d2 is not finite (a degenerate triangle that divides zero by zero) never wins.  The
 *   value is min(sqrt(min_t d2), band): far voxels hold exactly `band`.  The minimum does not depend on the order, so the
 *   broad phase (bricks of 8 x 8 x 4 voxels list the triangles whose box, inflated by the band, reaches them) gives the
 *   brute-force bits.
 *   Sign (flags & DSL_SDF_UNSIGNED == 0).  A voxel is inside when the ray from it towards +x crosses an odd number of
 *   triangles; the value is inside ? -d : d.  No normals, no orientation.  Projected onto (y, z): per edge of a triangle,
 *   its ends ordered by (y, then z) are lo and hi, delta = hi - lo, E(q) = delta.y (q.z - lo.z) - delta.z (q.y - lo.y).  A
 *   triangle is skipped when an edge has delta = 0 or E(r) is not > 0 or < 0 for the opposite vertex r.  The ray of the row
 *   (y, z) belongs to the triangle when y and z lie within the vertices' smallest and largest y and z and, for all three
 *   edges, sgn E(row) = sgn E(r), E(row) == 0 read as + when delta.z <= 0 and as - when delta.z > 0 (one infinitesimal shift
 *   of every ray: exactly one of two triangles across an edge claims a ray through it).  The crossing lies at
 *   x_hit = a.x - (n.y (y - a.y) + n.z (z - a.z)) / n.x, n = ab x ac, and counts for the voxels with x < x_hit.  An open
 *   mesh gives what the parity gives.
 *   DSL_ERR_INVALID (dsl_last_error names the argument), before anything is touched: T = 0 or more than 2^24, a NULL
 *   vertices / origin / step / dims, both outputs NULL, a dims entry < 1, more than 2^30 voxels, a step entry that is not
 *   finite and > 0, a non-finite origin, band not > 0 (+inf is allowed: every brick lists every triangle), unknown flags.
 *   DSL_K_SDF times every launch; DSL_OPT_SDF_* describe the last call.
 *
 * dsl_collider_set_volume: a distance volume (dsl_mesh_distance_volume's, or any the host computed) as the collider of the
 * step.  Exactly one of dev_volume and host_volume is given; the library copies it and owns the copy.  Blocking.
 * dims = NULL removes the collider.  DSL_ERR_INVALID: a dims entry < 2, more than 2^30 voxels, a bad step or origin as
 * above, both or neither pointer, unknown flags -- and a mesh collider that is set: a mesh and a volume exclude each other
 * (dsl_collider_set_mesh refuses likewise while a volume is set; remove the one before setting the other).
 * DSL_ERR_UNSUPPORTED: a slab handle; and a handle with a volume refuses dsl_slab_config.
 *   Rule, per fluid particle at x: u_a = (x_a - origin_a) / step_a, i_a = floor(u_a), t_a = u_a - i_a.  No collision when an
 *   i_a is outside [0, n_a - 2], a corner of the cell is not finite or x is not finite.  With lerp(p, q, t) = p + t (q - p):
 *   d = the trilinear interpolant of the eight corners, x first, then y, then z; the gradient g_a = (the bilinear
 *   interpolant of the cell's upper a-face - that of its lower a-face) / step_a, the faces interpolated in axis order
 *   (x before y before z); |g| = sqrt((g.x g.x + g.y g.y) + g.z g.z).  DSL_SDF_UNSIGNED in flags records that the volume is
 *   a thin shell; d and g are taken as they are either way.  The particle collides when d < radius and |g| > 0:
 *   n = g / |g|, x <- x + (radius - d) n and, when v.n < 0, v <- v - ((1 + restitution) (v.n)) n.  Boundary particles,
 *   the PCISPH predictor state and dsl_stats.max_vel / max_f are not touched.
 * While a volume is set dsl_collide_pass runs this pass, the step drivers run it where they run the mesh pass (after Update
 * in dsl_wcsph_step, dsl_pcisph_step and DSL_PCI_END_STEP) and the skin step is not taken.  DSL_OPT_COLLIDE_HITS counts the
 * particles moved, DSL_K_COLLIDE times the launch.  Without a volume: no launch, no bit changes.
 * dsl_collider_volume_query: d and n of every fluid particle in host order (zeros where there is no cell, a zero normal
 * where |g| is not > 0), no response, whatever the radius; either pointer may be NULL.  Blocking.  Not in slab mode.
 *
 * dsl_collider_volume_motion: the volume collider as a rigid body in motion.  The voxels stay in the body's own frame, where
 * they were built; the pose takes every particle into that frame and the normal back out of it.  rot: 9 floats, row-major R,
 * whose columns are the body's axes in world coordinates; trans: the body frame's origin in world coordinates; lin_vel,
 * ang_vel: the body's velocity at `trans` and its angular velocity, world.  A NULL pointer is the identity / zero; all four
 * NULL: motion off, the static pass runs again.  The call does not synchronise and touches no device memory: the 18
 * numbers go by value into each later launch, so a host calls it between steps as often as it likes.  The pose in force
 * when a step driver is called holds for all nsteps of that call -- the library does not integrate the pose; a host that
 * moves a body steps one at a time.  R is used as supplied, like the mesh collider's normals: not re-orthonormalised, not
 * checked beyond being finite.  DSL_ERR_INVALID (dsl_last_error names the argument): no volume collider is set, a value is
 * not finite.  DSL_ERR_UNSUPPORTED: a slab handle.  DSL_ERR_NOMEM: the sums' arrays (allocated when a motion is first set)
 * could not be had; motion stays off.  A refused call changes nothing.  dsl_collider_set_volume -- a new volume or the
 * removal -- turns motion off and zeroes the accumulators.  DSL_OPT_COLLIDER_VOLUME_MOVING is 1 while a motion is set.
 *   Rule, per fluid particle at x with velocity v; float32, every operation rounded once, nothing fused, a dot product is
 *   (a.x b.x + a.y b.y) + a.z b.z, the same in both math modes:  q = x - trans;  xl_a = (R[0][a] q.x + R[1][a] q.y) + R[2][a] q.z
 *   (R^T q);  cell, d, g, |g|: the rule above evaluated at xl ("x is not finite" is tested on xl);  nl = g / |g|;
 *   n_a = (R[a][0] nl.x + R[a][1] nl.y) + R[a][2] nl.z.  The particle collides when there is a cell, |g| > 0 and d < radius:
 *   x <- x + (radius - d) n.  The body's velocity at the particle is u = lin_vel + ang_vel x q:
 *   u.x = lin.x + (w.y q.z - w.z q.y), u.y and u.z its cyclic permutations, every product and difference rounded.
 *   vn = (v - u).n; when vn < 0: f = (1 + restitution) vn, v <- v - f n, and the body receives the impulse J = (mass f) n,
 *   mass f rounded first, and the torque impulse tau = q x J (tau.x = q.y J.z - q.z J.y and its cyclic permutations).  A
 *   particle that is only pushed out (vn >= 0) hands over nothing: the position correction carries no momentum.  With the
 *   identity, a zero translation and zero velocities every step is exact and the pass gives the static pass's bits.
 *   The sums are reproducible, no float atomics: two runs give the same bytes.  Per slot s, in the order dsl_download_ids
 *   reports, the contribution c_s has six components, J then tau, +0 for a slot that did not respond.  Workgroup b owns the
 *   slots [256 b, 256 b + 256), slots past the last live one counting as +0; its partial is the tree
 *   `for off in 128, 64, 32, 16, 8, 4, 2, 1: c[l] += c[l + off] for l < off`.  The pass total: lane l of one 256-lane
 *   workgroup adds the partials l, l + 256, l + 512, ... in ascending order, starting from +0, and the same tree combines the
 *   256 lane sums.  Then acc <- acc + total, once per pass, passes in stream order.
 * While a motion is set dsl_collide_pass and the step drivers run this pass and its fold where they run the static pass
 * (both timed under DSL_K_COLLIDE), and dsl_collider_volume_query returns d and the world-space n at the pose in force.
 * dsl_collider_volume_impulse: what the fluid handed to the body since the last reset: impulse (3) and torque impulse
 * about `trans` (3); either may be NULL.  Blocking.  reset = 1 zeroes the accumulators after the read.  Zeros while no
 * motion has been set.  Not in slab mode. */
#define DSL_SDF_UNSIGNED 1
int dsl_mesh_distance_volume(dsl_handle *h, const float *vertices /* 9*T, host */, size_t n_triangles,
                             const float origin[3], const float step[3], const int32_t dims[3],
                             float band, int flags, float *dev_out, float *host_out);
int dsl_collider_set_volume(dsl_handle *h, const float *dev_volume, const float *host_volume, const float origin[3],
                            const float step[3], const int32_t dims[3], float radius, float restitution, int flags);
int dsl_collider_volume_query(dsl_handle *h, float *dist /* N */, float *normal /* 3N */);
int dsl_collider_volume_motion(dsl_handle *h, const float rot[9], const float trans[3],
                               const float lin_vel[3], const float ang_vel[3]);
int dsl_collider_volume_impulse(dsl_handle *h, float impulse[3], float torque[3], int reset);

/* Rigid bodies: up to DSL_MAX_BODIES volume colliders, each with a pose of its own, and the poses integrated on the device
 * (csrc/bodies.hip; tests/bodies_ref.py restates the rule operation for operation).  The reference's
 * sph.Init(scl, origin, colliders []geom.Collider, ...) takes a list of colliders; this is that list for distance volumes.
 *
 * dsl_body_add: a body from a distance volume (exactly one of dev_volume / host_volume; the library copies it; the lattice
 * is checked as dsl_collider_set_volume checks it, dims >= 2), its properties and its first state (NULL: the identity, at
 * rest).  Bodies get the ids 0, 1, ... in the order they were added (*body_id, may be NULL).  Blocking.  There is no removal
 * of one body, because the order is part of the rule; dsl_bodies_clear removes all of them (blocking).  Without bodies
 * there is no launch and no bit changes.  The copies, the body records, the partial sums and the accumulators are the
 * library's own: counted in DSL_OPT_DEVICE_BYTES, freed by dsl_bodies_clear and dsl_destroy.
 *   dsl_body_props: inv_mass and inv_inertia (the inverse principal moments, about the axes of the body's frame) turn what
 *   the fluid hands over into velocity; accel is a constant acceleration (gravity); radius and restitution are the
 *   collider's.  inv_mass = 0, inv_inertia = 0 and accel = 0: a kinematic body, which moves with its velocities and ignores
 *   the fluid.
 *   dsl_body_state: quat (w, x, y, z) is the orientation, trans the body frame's origin in world coordinates -- the point
 *   torques refer to, so a caller puts it at the centre of mass -- lin_vel the velocity of that point, ang_vel the
 *   angular velocity, world.  The voxels stay in the body's frame.
 * dsl_body_set_state / dsl_body_set_props replace one of the two between steps and take effect at the next pass (blocking);
 * dsl_body_get_state reads the state and what the fluid handed to the body since the last reset (impulse, torque impulse
 * about trans; any of the three pointers may be NULL; reset = 1 zeroes the accumulators after the read); blocking.
 * dsl_body_query: d and the world-space n of every fluid particle in host order against one body at its current pose, no
 * response, as dsl_collider_volume_query; blocking.
 *   DSL_ERR_INVALID (dsl_last_error names the argument), before anything is touched, a refused call changes nothing: a
 *   seventeenth body, a bad lattice or bad pointers, a non-finite entry anywhere, inv_mass, an inv_inertia entry or radius
 *   < 0, a quaternion whose squared length is not > 0 (or not finite), an unknown body id; dsl_body_add while a mesh
 *   collider or the single volume collider is set -- and dsl_collider_set_mesh / dsl_collider_set_volume while bodies
 *   exist: the three kinds of collider exclude each other, and the message says what to remove first.
 *   DSL_ERR_UNSUPPORTED: a slab handle; dsl_slab_config refuses while bodies exist.  The skin step is not taken while
 *   bodies exist.  dsl_stats.max_vel / max_f, boundary particles and the PCISPH predictor state are not touched.
 *   Rule.  float32, every operation rounded once, nothing fused, a dot product is (a.x b.x + a.y b.y) + a.z b.z, divisions
 *   and square roots correctly rounded, the same in both math modes.
 *   Pose.  dsl_body_set_state (and dsl_body_add) store q / |q|, |q| = sqrt(((w w + x x) + y y) + z z), each component
 *   divided, and derive the row-major R = [1 - 2 (yy + zz), 2 (xy - wz), 2 (xz + wy);  2 (xy + wz), 1 - 2 (xx + zz),
 *   2 (yz - wx);  2 (xz - wy), 2 (yz + wx), 1 - 2 (xx + yy)], every product, sum and difference rounded, each parenthesis
 *   formed first.
 *   Pass.  For every live fluid slot, in dsl_download_ids order, body 0, then 1, ..., then K - 1, in that order: the rule of
 *   dsl_collider_volume_motion above (q, xl = R^T q, cell, d, g, n = R nl, push-out, u, vn, f, J = (mass f) n, tau = q x J)
 *   with that body's radius, restitution, R, trans, lin_vel and ang_vel, applied to the particle's current x and v: body 1
 *   sees what body 0 left.  A body's contribution from a slot is J, tau, or six +0.  Per body the workgroup partials (256
 *   slots, the same tree) and the pass total are those of dsl_collider_volume_motion; then acc_b <- acc_b + total_b.
 *   DSL_OPT_COLLIDE_HITS counts the moved (particle, body) pairs of the last pass.
 *   Integration.  Only in the step drivers (dsl_wcsph_step, dsl_pcisph_step, DSL_PCI_END_STEP), after each step's fold, and
 *   only while DSL_OPT_BODIES_INTEGRATE is 1; dsl_collide_pass runs the pass and the fold alone.  dt = dsl_params.dt.  Per
 *   body, (J, tau) = total_b of this pass, R the pose the pass used, a over the three axes:
 *     1. lin_a <- lin_a + (J_a inv_mass + accel_a dt)
 *     2. tl = R^T tau;  wl_a = tl_a inv_inertia_a;  ang <- ang + R wl   (the two matrix products row by dot product)
 *     3. trans_a <- trans_a + dt lin_a   (the new lin)
 *     4. with w = the new ang: dw = -((w.x q.x + w.y q.y) + w.z q.z),  dx = q.w w.x + (w.y q.z - w.z q.y),
 *        dy = q.w w.y + (w.z q.x - w.x q.z),  dz = q.w w.z + (w.x q.y - w.y q.x),  hd = 0.5 dt
 *     5. q' = q + hd (dw, dx, dy, dz) per component;  q <- q' / |q'|;  R from q.
 *   There is no gyroscopic term (w x I w is left out: the inertia acts as if the body's axes were principal and the spin
 *   slow against the step).  At the identity, at rest, with zeros everywhere every step is exact: q stays (1, 0, 0, 0),
 *   R the exact identity, and the pass gives the static pass's bits.
 * Both launches of a pass (the pass; the fold with the integration as its last act) are timed under DSL_K_COLLIDE. */
#define DSL_MAX_BODIES 16
typedef struct dsl_body_props {
  float inv_mass;
  float inv_inertia[3];
  float accel[3];
  float radius;
  float restitution;
} dsl_body_props;
typedef struct dsl_body_state {
  float quat[4]; /* w, x, y, z */
  float trans[3];
  float lin_vel[3];
  float ang_vel[3];
} dsl_body_state;
int dsl_body_add(dsl_handle *h, const float *dev_volume, const float *host_volume, const float origin[3], const float step[3],
                 const int32_t dims[3], const dsl_body_props *props, const dsl_body_state *state, int *body_id);
int dsl_bodies_clear(dsl_handle *h);
int dsl_body_set_state(dsl_handle *h, int body, const dsl_body_state *state);
int dsl_body_set_props(dsl_handle *h, int body, const dsl_body_props *props);
int dsl_body_get_state(dsl_handle *h, int body, dsl_body_state *state, float impulse[3], float torque[3], int reset);
int dsl_body_query(dsl_handle *h, int body, float *dist /* N */, float *normal /* 3N */);

/* Contact of the rigid bodies with the wall box and with each other (csrc/contact.hip; tests/contact_ref.py restates the rule
 * operation for operation).  Opt-in: DSL_OPT_BODIES_CONTACT (default 0) is bit 1 (walls) | bit 2 (bodies).  While it is 0 and
 * none of the three calls below is made, nothing changes: no launch, no allocation, no bit.  The rule is build-defined, with
 * the arithmetic conventions of the bodies' rule above (float32, one rounding per operation, nothing fused, the ordered dot
 * product, (u x v).x = u.y v.z - u.z v.y and cyclic with each product and difference rounded, `/` and sqrt correctly
 * rounded), the same in both math modes.
 *   Contact points.  A voxel of a body's volume is a contact point when its value is finite and <= 0 and at least one of
 *   its up to six axis neighbours inside the lattice is finite and > 0: the innermost shell.  A body's list is the set of
 *   such voxels as int32 linear indices (x fastest), ascending, built on the device from the library's copy of the volume by
 *   a count, a prefix sum and an emit.  A point's body-frame coordinate is origin + step * (float)index per axis, the rule
 *   of dsl_field_volume.  An unsigned (thin-shell) volume has no point: such a body never initiates a contact (and, d < 0
 *   never holding in it, no other body's point finds it: only the fluid does).  The lists are built for all bodies when the
 *   option first becomes non-zero or one of the calls below first needs them, and at dsl_body_add while the option is
 *   non-zero -- never at dsl_body_add while it is 0.  dsl_body_add builds the list before the body exists: if that fails
 *   (DSL_ERR_NOMEM) there is no new body.  They, the partial sums and the table are counted in DSL_OPT_DEVICE_BYTES and freed
 *   by dsl_bodies_clear and dsl_destroy.
 *   Detection.  For every body A at its current pose (R, trans) and every point pl of A: q_a = (R[a][0] pl.x + R[a][1] pl.y)
 *   + R[a][2] pl.z, x_a = trans_a + q_a.  Each body has 6 + K targets.  Wall target t = 2 a + side, only with bit 1 and
 *   dsl_params.walls != 0: side 0: pen = box_min[a] - x_a, n = +e_a; side 1: pen = x_a - box_max[a], n = -e_a; the point
 *   contributes when pen > 0.  Body target t = 6 + B, B != A, only with bit 2: the bodies' pass's evaluation of x against B
 *   (r = x - trans_B, xl = R_B^T r, the cell, d, g, n = R_B (g / |g|)); the point contributes when there is a cell, |g| > 0
 *   and d < 0, with pen = -d.  No bounding test skips a body.  A contribution is the eight sums (pen q.x, pen q.y, pen q.z,
 *   pen n.x, pen n.y, pen n.z, pen, 1) and the depth pen; a point that does not contribute gives nine +0.  Per (A, t):
 *   workgroup b owns points [256 b, 256 b + 256) of A's list and reduces the sums with the tree of
 *   dsl_collider_volume_motion; the total adds the partials lane-strided and ascending from +0, then the same tree over the
 *   256 lane sums; the depth D is the maximum.  No float atomics.  The table is E[A][t] = (S[3], N[3], W, C, D): nine
 *   floats per entry, K (6 + K) entries, nine +0 for t = 6 + A and for a kind that is off.
 *   Solve.  One lane, A ascending and inside A t ascending, every quantity of a body read from its record as the earlier
 *   contacts of this solve left it.  An entry is skipped unless W > 0.  qc_a = S_a / W.  Wall: n is the axis vector.  Body:
 *   len = sqrt(dot3(N, N)), skipped unless len > 0, n_a = N_a / len.  Iw_X(t) is the integration's step 2: tl = R^T t,
 *   wl_a = tl_a inv_inertia_a, R wl.  tA = Iw_A(qc x n), kA = inv_mass_A + dot3(tA x qc, n).  Body target:
 *   rB_a = (trans_A_a + qc_a) - trans_B_a, tB = Iw_B(rB x n), kB = inv_mass_B + dot3(tB x rB, n), k = kA + kB; wall: k = kA.
 *   Skipped unless k > 0: a kinematic body is moved by nothing, but others bounce off it.  uA = lin_A + ang_A x qc,
 *   uB = lin_B + ang_B x rB (0 for a wall), vn = dot3(uA - uB, n).  When vn < 0: e = A's restitution against a wall, fminf
 *   of the two against a body; f = (1 + e) vn; j = (-f) / k; lin_A_a += (j inv_mass_A) n_a; ang_A_a += j tA_a;
 *   lin_B_a -= (j inv_mass_B) n_a; ang_B_a -= j tB_a.  Push-out against a wall, when inv_mass_A > 0: trans_A_a += D n_a.
 *   Against a body, with s = inv_mass_A + inv_mass_B, when s > 0: trans_A_a += ((0.5 D)(inv_mass_A / s)) n_a,
 *   trans_B_a -= ((0.5 D)(inv_mass_B / s)) n_a -- the half because the pair is met twice, as (A, B) and as (B, A).  The
 *   quaternion and R are not touched.
 *   Limits.  There is no friction and no stacking solver; a body rests with its innermost voxel shell on the wall; a body
 *   that moves more than its own thickness per step tunnels; contact between bodies reaches as deep as B's band, because
 *   beyond it |g| = 0.
 *   Where it runs.  Only in the step drivers (dsl_wcsph_step, dsl_pcisph_step, DSL_PCI_END_STEP), after each step's fold and
 *   integration, only while DSL_OPT_BODIES_INTEGRATE is 1 and DSL_OPT_BODIES_CONTACT is non-zero: pass, fold + integrate,
 *   detect, table fold, solve; the contact launches are timed under DSL_K_COLLIDE.  dsl_collide_pass stays as it is.
 * dsl_contact_points: the first min(M, cap) voxel indices of a body's list and M (*count, may be NULL); cap = 0 with a NULL
 *   array is the counting call.  Blocking.
 * dsl_contact_pass: detection at the current poses for `kinds` (bit 1 | bit 2), whatever the option is; solve != 0 adds the
 *   solve.  Asynchronous -- but the first call after bodies were added (and, likewise, the first step of a step driver with
 *   the option on) blocks: it builds the lists that are missing and lays out the detection's grid, with two stream
 *   synchronisations.  DSL_ERR_INVALID: no bodies, or unknown kinds.
 * dsl_contact_table: the last detection's 9 K (6 + K) floats; count must match.  Blocking.
 * All three: DSL_ERR_UNSUPPORTED on a slab handle; an unknown body id is refused as in dsl_body_query; a refused call changes
 * nothing. */
int dsl_contact_points(dsl_handle *h, int body, int32_t *host_voxels, size_t cap, int64_t *count);
int dsl_contact_pass(dsl_handle *h, int kinds, int solve);
int dsl_contact_table(dsl_handle *h, float *host, size_t count);

/* Sources and sinks: fluid particles created and removed on the device, so the particle count of a handle changes between
 * steps.  The rule is build-defined (the reference has no sources; tests/sources_ref.py restates it operation for operation)
 * and the same in both math modes.
 *
 * A new particle -- appended by the host or emitted -- takes the next host index N (the indices run on: N .. N + n_new - 1) and
 *   has the given position and velocity, force = force_reset, pressure 0, density 0 and P/rho^2 0 (what a fresh handle's
 *   zero-filled arrays read) until the next density pass, and, while PCISPH is active, predictor state equal to its position
 *   and velocity (what dsl_pcisph_begin would copy).  Forces that are not uniform are kept: force_reset goes into the new
 *   slots of the array.  The neighbour table is stale afterwards; densities stay on their particles.  dsl_get_params returns
 *   the new n_particles and dsl_set_params accepts exactly it.
 * A layer of an emitter: lattice point (a, b) of the face, 0 <= a < nu, 0 <= b < nv, lies at
 *   (origin_c + (float)a * u_c) + (float)b * v_c per component c, every product and sum rounded once to float32, never fused
 *   (dsl_field_volume's discipline: a caller reproduces every bit).  shape 0 keeps every point; shape 1, the ellipse inscribed
 *   in the rectangle, keeps (a, b) when (2a - (nu-1))^2 nv^2 + (2b - (nv-1))^2 nu^2 <= (nu nv)^2 in 64-bit integers (the
 *   centre is always kept).  The kept points, b ascending and inside it a ascending, are the layer: M particles with host
 *   indices N .. N + M - 1 in that order, every one with the emitter's velocity.
 * The schedule: at the start of step s (s = dsl_stats.steps before the step) the step drivers dsl_wcsph_step,
 *   dsl_pcisph_step and DSL_PCI_BEGIN_STEP first apply the sinks when DSL_OPT_SINK_EVERY is not 0 and s % every == 0, then
 *   visit the emitters in ascending id: emitter e emits one layer when s >= first_step, (s - first_step) % period == 0 and
 *   it has emitted fewer than max_layers layers (max_layers 0: no limit).  A layer that does not fit dsl_params.capacity is
 *   skipped whole -- never a partial layer, never an error from the step; DSL_OPT_EMIT_SKIPPED counts it and it does not
 *   count towards max_layers.  All of it happens at step counts fixed in advance: results do not depend on how the steps were
 *   grouped into calls.  Emission needs no synchronisation (the host knows every count); a look of the sinks is one count
 *   kernel and one 4-byte read-back, and the compaction runs only when the count is not 0.
 * A sink is a box: inside = (x_a >= box_min_a && x_a < box_max_a) on all three axes (entries may be +-infinity, a NaN
 *   coordinate is never inside); a particle goes when, for some sink, inside != (outside != 0).  Survivors keep their
 *   relative host order -- the new host index of a survivor is the number of survivors with a smaller old index -- and every
 *   per-particle buffer follows its particle: positions, velocities, forces, densities, pressures, the PCISPH predictor
 *   state.  Densities keep their standing (held, and fresh if they were); the neighbour table is stale.  The slot order
 *   afterwards is the library's choice (dsl_download_ids describes it).  A handle is never emptied: when every particle
 *   would go, the one with the smallest host index stays.
 *
 * dsl_particles_append: n_new particles from host arrays of 3 n_new floats (host_velocities NULL: zeros).  Blocking.
 *   DSL_ERR_NOMEM (dsl_last_error names capacity) when N + n_new > capacity; DSL_ERR_INVALID on a NULL array, n_new = 0 or
 *   a non-finite entry.
 * dsl_emitter_add: up to DSL_MAX_EMITTERS; *id (may be NULL) is the emitter's index.  Blocking: it builds the list of kept
 *   points on the host and uploads it, one int32 word per point (counted in DSL_OPT_DEVICE_BYTES).  DSL_ERR_INVALID
 *   (dsl_last_error names the field): a ninth emitter, nu, nv or period < 1, nu * nv > 2^20, u or v all zero, a non-finite
 *   entry, first_step or max_layers < 0, an unknown shape.  dsl_emitters_clear removes all of them and frees the lists.
 * dsl_emit: one layer of emitter `emitter` now, between steps, for a host that drives the passes itself; it counts towards
 *   max_layers (DSL_ERR_INVALID once they are used up, or for an unknown id) and a layer that does not fit is refused with
 *   DSL_ERR_NOMEM.  Asynchronous.
 * dsl_sink_add: up to DSL_MAX_SINKS.  DSL_ERR_INVALID: a ninth sink, a NaN entry, box_min > box_max.  dsl_sinks_clear
 *   removes all of them.
 * dsl_particles_remove: applies the sinks now; *removed (may be NULL) is the number of particles that went.  Blocking.
 *
 * DSL_ERR_UNSUPPORTED from all of them but the two clear calls, with dsl_last_error naming what to remove first: a slab
 * handle (and dsl_slab_config refuses while emitters or sinks exist), DSL_NEIGH_LSH_REF, a handle with boundary particles
 * (fluid stays in front; dsl_add_boundary_particles refuses while emitters or sinks exist and once the count has changed),
 * after dsl_set_ids.  While the caller's stream is being captured a step that would emit or look returns
 * DSL_ERR_UNSUPPORTED: a replayed graph cannot change its grids or wait for a read-back.  A refused call changes nothing.
 * The skin step is not taken while an emitter or a sink exists.  Colliders, bodies, contact, field operators, volumes and
 * surfaces work on the count of the moment.  Limits: no jitter and no test for fluid in front of a face (a host that wants
 * either appends itself); dt is constant, so the spacing of the layers, period * dt * |velocity|, is the host's arithmetic;
 * no sources on slab ranks.  Every launch is timed under DSL_K_SOURCES.  With no emitter, no sink and none of these calls
 * made: no launch, no allocation, no bit changes. */
#define DSL_MAX_EMITTERS 8
#define DSL_MAX_SINKS 8
typedef struct dsl_emitter {
  float origin[3], u[3], v[3]; /* lattice point (a, b) of the face: origin + a u + b v, world */
  int32_t nu, nv;              /* 1 <= nu, nv; nu * nv <= 2^20 */
  int32_t shape;               /* 0 rectangle, 1 ellipse inscribed in it */
  float velocity[3];           /* every emitted particle starts with it */
  int32_t period;              /* >= 1: a layer every period-th step */
  int64_t first_step;          /* absolute, on the handle's step counter (dsl_stats.steps) */
  int64_t max_layers;          /* 0: no limit */
} dsl_emitter;
typedef struct dsl_sink {
  float box_min[3], box_max[3];
  int32_t outside; /* 0: particles inside the box go; otherwise: particles outside it */
} dsl_sink;
int dsl_particles_append(dsl_handle *h, const float *host_positions, const float *host_velocities, size_t n_new);
int dsl_emitter_add(dsl_handle *h, const dsl_emitter *emitter, int *id);
int dsl_emitters_clear(dsl_handle *h);
int dsl_emit(dsl_handle *h, int emitter);
int dsl_sink_add(dsl_handle *h, const dsl_sink *sink, int *id);
int dsl_sinks_clear(dsl_handle *h);
int dsl_particles_remove(dsl_handle *h, int64_t *removed);

/* The frame recorder: animation frames packed on the device during a run ("Fluid Animation Export", README.MD:39; the
 * reference reads every position back after every step and blocks, pcisph_gpu_darwin.go:276-279).  A recorder makes the step
 * drivers capture a frame every `every`-th step: two small launches reduce the captured particles' bounds, one packs the
 * frame -- host order, every stride-th particle, float32 or 16-bit -- into a staging frame in device memory, and one
 * hipMemcpyAsync on a copy stream of the library's own moves it to a slot of pinned host memory behind the steps that follow.
 * The step stream never waits for the host; it waits on the device only when both staging frames still have their copies
 * outstanding.  The skin step stays on: the pack reads the slot -> particle map where it lives, on the device.  The rule is
 * build-defined (tests/record_ref.py restates it operation for operation) and the same in both math modes.
 *
 * A frame is self-describing, little-endian: a 128-byte header, then the planes, each starting at the next multiple of 128
 * bytes; frame_bytes is the end of the last plane rounded up to a multiple of 128, and the padding is zero.  The header:
 *     0 u32 magic 0x464C5344 ("DSLF")     4 u32 128 (the header's size)     8 u64 frame_bytes     16 i64 step
 *    24 i32 n_particles (N at that step)  28 i32 count M = ceil(N / stride) 32 i32 stride         36 i32 fields
 *    40 i32 encoding    44 i32 auto_box (1 or 0; 0 for F32)   48 f32[3] box_min   60 f32[3] box_max (the box Q16 was encoded against; zeros for F32)
 *    72 f32[3] bounds_min   84 f32[3] bounds_max   96 f32 dt   100 i32 finite   104 .. 127 zero
 * The planes: positions, then velocities if DSL_REC_VELOCITY, then densities if DSL_REC_DENSITY; xyz interleaved, entry m
 *   belongs to host index m * stride; fluid particles only.  DSL_REC_F32: 12 M, 12 M and 4 M bytes of float32, bit for bit what
 *   dsl_download / dsl_download_decimated would return at that moment (densities: those the last density pass left, zeros on
 *   a fresh handle).  DSL_REC_Q16: 6 M bytes of uint16 x 3, 6 M of float16 x 3, 2 M of float16.
 * The bounds run over the captured particles whose three coordinates are finite; `finite` is their number.  Minimum and
 *   maximum are those of the total order of the key bits ^ (bits >> 31 ? 0xffffffff : 0x80000000) on the float's bits, so -0
 *   lies below +0; with no finite particle they are +inf / -inf.  (Minimum, maximum and an integer count do not depend on the
 *   order of a reduction: any order gives the same bits.)
 * DSL_REC_Q16, per axis, against the box [lo, hi] -- the spec's box_min / box_max, or with auto_box the frame's own bounds:
 *   scale = 65535.0f / (hi - lo) when hi - lo is finite and > 0, else 0 (one rounded subtraction, one correctly rounded
 *   division); t = (x - lo) * scale, each operation rounded once, nothing fused; r = rintf(t) (ties to even);
 *   q = r >= 65535 ? 65535 : (r > 0 ? r : 0), so a NaN gives 0.  A reader decodes lo + q * ((hi - lo) / 65535).  Velocities
 *   and densities: float32 -> float16, round to nearest even, subnormal results and overflow to infinity as IEEE 754 has
 *   them; a NaN keeps its sign and its ten top payload bits, 0x7c01 where those are zero (every bit pattern: numpy's
 *   astype(float16)).
 * The schedule: frame s is the state when dsl_stats.steps == s, before anything of step s, this step's sinks and emitters
 *   included.  dsl_wcsph_step, dsl_pcisph_step and DSL_PCI_BEGIN_STEP capture it when s >= first_step,
 *   (s - first_step) % every == 0 and fewer than max_frames frames were recorded (0: no limit): results do not depend on how
 *   the steps were grouped into calls.
 * The ring: `slots` frames of pinned host memory, each dsl_record_frame_bytes(spec, capacity) bytes (sources change N).  A
 *   frame that finds no RELEASED slot is dropped whole and counted (DSL_OPT_RECORD_DROPPED); it does not count towards
 *   max_frames.  Release is a host call, so what is dropped does not depend on timing.  Frames come out in FIFO order.
 *
 * dsl_recorder_set: stores the spec and allocates -- at most two staging frames in device memory (counted in
 *   DSL_OPT_DEVICE_BYTES) and the pinned slots.  Blocking.  NULL: the recorder is off and everything is freed (unread frames
 *   go with it).  A new spec replaces the old recorder and its frames.  DSL_ERR_INVALID (dsl_last_error names the field):
 *   every, stride < 1, slots outside 1 .. 64, first_step or max_frames < 0, unknown field bits or encoding, and for
 *   DSL_REC_Q16 without auto_box a box that is not finite or has box_min > box_max.  DSL_ERR_UNSUPPORTED: a slab handle (and
 *   dsl_slab_config refuses while a recorder is set), after dsl_set_ids (host order is gone).  DSL_ERR_NOMEM when pinned or
 *   device memory cannot be had: the handle stays usable, without a recorder.
 * dsl_record_frame_bytes: the size of a frame of n_particles particles under the spec; 0 for a spec dsl_recorder_set would
 *   refuse or n_particles < 1.
 * dsl_record_now: one frame of the current state, between steps (its step field is dsl_stats.steps), for a host that drives
 *   the passes itself.  It obeys the same ring (DSL_ERR_NOMEM when no slot is released) and counts towards max_frames
 *   (DSL_ERR_INVALID once they are used up).  Asynchronous; like every entry point but the step drivers it settles a live
 *   skin episode.
 * dsl_record_poll: frames recorded so far, frames whose copy has landed and that are not yet released, frames dropped; any
 *   pointer may be NULL.  Never blocks.  (dsl_sync waits for the copies on their way as well as for the steps.)
 * dsl_record_peek: the oldest unreleased frame in its pinned slot and its size; waits for ITS copy only.  The pointer stays
 *   valid and the bytes unchanged until dsl_record_release, which hands the slot back.  dsl_record_read: peek, memcpy into
 *   host_out (bytes: its size, at least the frame's), release.  DSL_ERR_INVALID from the three with nothing to give, or for
 *   a `bytes` that is too small.
 *
 * A refused call changes nothing.  While the caller's stream is being captured a step that would record returns
 * DSL_ERR_UNSUPPORTED.  DSL_NEIGH_LSH_REF, boundary particles (never recorded), colliders, bodies and sources all work.  Not
 * recorded: forces and pressures (held lazily), the extracted surface; no crop box; no recording on slab ranks.  With no
 * recorder set: no launch, no allocation, no bit changes. */
#define DSL_REC_VELOCITY 1 /* fields: positions always, | velocities | densities */
#define DSL_REC_DENSITY 2
enum { DSL_REC_F32 = 0, DSL_REC_Q16 = 1 };
typedef struct dsl_recorder {
  int32_t every;    /* >= 1: a frame at steps s >= first_step with (s - first_step) % every == 0 */
  int32_t stride;   /* >= 1: host indices 0, stride, 2 stride, ... (dsl_download_decimated's) */
  int32_t fields, encoding;
  int32_t slots;    /* 1..64 frames of pinned host memory */
  int32_t auto_box; /* Q16: 0 = box_min/box_max below, 1 = each frame's own bounds */
  float box_min[3], box_max[3];
  int64_t first_step; /* absolute, on dsl_stats.steps */
  int64_t max_frames; /* 0: no limit */
} dsl_recorder;
int dsl_recorder_set(dsl_handle *h, const dsl_recorder *spec);
size_t dsl_record_frame_bytes(const dsl_recorder *spec, int n_particles);
int dsl_record_now(dsl_handle *h);
int dsl_record_poll(dsl_handle *h, int64_t *recorded, int64_t *ready, int64_t *dropped);
int dsl_record_peek(dsl_handle *h, const void **frame, size_t *bytes);
int dsl_record_release(dsl_handle *h);
int dsl_record_read(dsl_handle *h, void *host_out, size_t bytes);

int dsl_get_stats(dsl_handle *h, dsl_stats *out);
int dsl_sync(dsl_handle *h); /* Queue.Finish() pcisph_gpu_darwin.go:261,271 */

/* Run on an existing hipStream_t (e.g. the caller framework's current stream) so that the
 * caller's copies/collectives and the engine's kernels are ordered.  NULL is HIP's default
 * stream.  dsl_use_own_stream goes back to the handle's private non-blocking stream. */
int dsl_set_stream(dsl_handle *h, void *hip_stream);
int dsl_use_own_stream(dsl_handle *h);

/* Per-kernel device timing with HIP events recorded on the launch stream.  on = 1: every kernel
 * (1.8 % of a 2.5 ms step at 16M particles, ~10 % of a 0.5 ms slab step); on = 2: only the
 * dominant kernels of a step (DSL_K_DENSITY, DSL_K_FORCE_INTEGRATE, DSL_K_PCI_DENSITY); 0: off. */
int dsl_timing_enable(dsl_handle *h, int on);
int dsl_timing_reset(dsl_handle *h);
int dsl_timing_get(dsl_handle *h, int kernel_id, double *avg_ms, int64_t *launches);

/* Debug/parity aid: state in the device's current (cell-sorted) order.
 * ids[s] is the original particle index held by slot s. */
int dsl_download_sorted(dsl_handle *h, int buffer, float *host, size_t count);
int dsl_download_ids(dsl_handle *h, int32_t *ids, size_t count);
int dsl_download_cell_start(dsl_handle *h, int32_t *cell_start, size_t count);

/* ---- multi-GPU: spatial slabs, one process per GPU -----------------------------------
 * The reference has no multi-process path; these entry points are
 * what a host needs to run one slab per GPU and exchange a halo with its two neighbours
 * (over RCCL, by whatever transport the host owns).
 *
 * A message is a DEVICE buffer of dsl_slab_message_floats(cap_full, cap_xonly) floats:
 *   header  : 7 words; [0] = number of full records, [1] = number of position-only records
 *             (int32 bits)
 *   full    : cap_full records of 7 floats: x,y,z,vx,vy,vz and the global particle id as
 *             raw int32 bits -- every owned particle within width_full of the plane, and the
 *             migrants beyond it
 *   x-only  : cap_xonly records of 4 floats: x,y,z and the global id (int32 bits) -- the rest of the
 *             band (out to `width`); they only feed the receiver's ghost densities.  The id keeps
 *             every cell of every rank in the order of a single-domain run (ascending id), which is
 *             what makes DSL_MATH_EXACT slabs bit-identical to it
 * Messages have a fixed size, so a step needs no host-side counts and no host
 * synchronisation: the live particle count stays on the device.  With width_full = h and
 * width = 2h the receiver recomputes the ghosts' densities itself and the force pass needs
 * no second exchange.
 *
 * dsl_slab_config : this handle owns [lo,hi) along `axis` (use -INFINITY / INFINITY at the
 *                   domain ends); particles outside are ghosts: they take part in the
 *                   neighbour sums but are not integrated and are dropped at the next
 *                   neighbour build.
 * dsl_slab_pack   : packs the bands of both sides (either pointer may be NULL) from the
 *                   current state.  Asynchronous.
 * dsl_slab_append : appends the records of a received message behind the current
 *                   particles; full records are owned if inside [lo,hi), ghosts otherwise.
 *                   Asynchronous.
 * dsl_slab_status : [0] largest count that did not fit a message or the particle capacity
 *                   since creation (0 = none), [1] 1 if the split step's margin was ever
 *                   exceeded, [2],[3] largest full / position-only band counts since the last
 *                   reset; blocking.  dsl_slab_overflow returns [0] only.
 * After appending, dsl_build_neighbours drops the previous step's ghosts (the integrate
 * kernels mark them with NaN positions).  A particle that has just crossed the plane stays
 * one more step as a ghost of its old owner.
 *
 * Split step (hides the exchange behind the interior force pass; DSL_MATH_FAST only):
 *   dsl_slab_split(h, width, margin) once; then per step, after the density pass,
 *   dsl_force_pass_split(h, DSL_SPLIT_BAND)   force+integrate for the particles of the grid-cell
 *                                             layers that reach within width+margin of a plane,
 *   dsl_slab_pack_band(h, ..., stream)        packs the integrated band.  stream = NULL: on the
 *                                             handle's stream, between the two launches (three
 *                                             small kernels, 25 us; the host then lets its
 *                                             transfer stream wait for that point).  A side
 *                                             stream is made to wait for the band phase only,
 *                                             but small kernels issued next to the interior
 *                                             launch are starved by it (two of its workgroups
 *                                             fill a CU's vector registers).
 *   dsl_force_pass_split(h, DSL_SPLIT_INNER)  the remaining layers, concurrently with the
 *                                             transfer the host started on `stream`.
 *   `margin` must exceed the distance a particle can move in one step (dsl_slab_status[1]
 *   reports a violation). */
enum { DSL_SPLIT_BAND = 1, DSL_SPLIT_INNER = 2 };
size_t dsl_slab_message_floats(int cap_full, int cap_xonly);
/* Once dsl_pcisph_begin has run, a full record also carries the predictor state (_pos, _vel of
 * pcisph_darwin.go:28-41, which the reference never re-synchronises): 13 floats instead of 7. */
int dsl_slab_record_floats(dsl_handle *h);
size_t dsl_slab_message_floats_for(dsl_handle *h, int cap_full, int cap_xonly);
int dsl_slab_config(dsl_handle *h, int axis, float lo, float hi);
int dsl_slab_split(dsl_handle *h, float width, float margin);
int dsl_slab_pack(dsl_handle *h, float width_full, float width, float *dev_lo, float *dev_hi, int cap_full,
                  int cap_xonly);
int dsl_slab_pack_band(dsl_handle *h, float width_full, float *dev_lo, float *dev_hi, int cap_full, int cap_xonly,
                       void *stream);
int dsl_force_pass_split(dsl_handle *h, int phase);
int dsl_slab_append(dsl_handle *h, const float *dev_message, int cap_full, int cap_xonly);
/* both neighbours' messages in one launch (either may be NULL); b lands behind a */
int dsl_slab_append2(dsl_handle *h, const float *dev_message_a, const float *dev_message_b, int cap_full,
                     int cap_xonly);
int dsl_slab_status(dsl_handle *h, int32_t status[4], int reset_high_water);
int dsl_slab_overflow(dsl_handle *h, int *high_water);
int dsl_get_count(dsl_handle *h, int *n_live, int *n_owned); /* blocking */
/* ---- multi-GPU: the exchange itself, behind the C ABI --------------------------------
 * The reference's only device host is Go (pcisph_gpu_darwin.go:249-286 drives one OpenCL queue); for
 * it to run N > 1 GPUs the halo exchange cannot live in some other language's runtime.  These entry
 * points own an RCCL communicator (bound at run time with dlopen: a single-GPU host never loads
 * RCCL) and drive the whole slab step, transfers included.
 *
 * dsl_comm_unique_id / dsl_comm_create : ncclGetUniqueId on one rank, its 128 bytes handed to every
 *                      rank by whatever channel the host owns (a Go channel, a socket, an MPI or
 *                      torch.distributed broadcast), then ncclCommInitRank; one process per GPU.
 * dsl_comm_create_all / dsl_create_multi : one process, `ndev` devices: ncclCommInitAll, resp. ndev
 *                      handles plus their communicators.  RCCL then wants ONE HOST THREAD PER DEVICE for
 *                      the step drivers below (a goroutine under runtime.LockOSThread each).
 * dsl_slab_attach    : after dsl_slab_config: neighbour ranks (-1 at a domain end), band widths,
 *                      message capacities (they may grow to twice these; identical on every rank),
 *                      overlap = 1 for the split step.  Allocates the message buffers and the
 *                      transfer stream.
 * dsl_slab_exchange  : pack both bands, ncclGroupStart / ncclSend + ncclRecv per neighbour /
 *                      ncclGroupEnd, append.  Asynchronous.
 * dsl_slab_wcsph_step / dsl_slab_pcisph_step : the slab step, nsteps times: exchange for the next
 *                      step at the end of each step (with overlap: band layers first, their pack and
 *                      the transfer on a side stream under the interior force launch); PCISPH adds
 *                      one 4-byte MAX all-reduce of the iteration error per correction iteration.
 *                      While a collider mesh is set (DSL_OPT_COLLIDE_SLAB) the collide pass follows every
 *                      integrate and precedes the pack behind it (see dsl_collide_pass).
 *                      Every 8th step the band high-water marks of all ranks are MAX-reduced (one
 *                      host synchronisation) and every rank switches to the same new message
 *                      sizes; an overflow or an outrun split margin ANYWHERE makes the call fail with
 *                      DSL_ERR_OVERFLOW on every rank instead of silently losing particles.
 * dsl_slab_replan    : that re-plan on demand (blocking, collective). */
#define DSL_COMM_ID_BYTES 128
typedef struct dsl_comm dsl_comm;
int dsl_comm_unique_id(uint8_t id[DSL_COMM_ID_BYTES]);
int dsl_comm_create(int nranks, int rank, const uint8_t id[DSL_COMM_ID_BYTES], int device, dsl_comm **out);
int dsl_comm_create_all(int ndev, const int *devices, dsl_comm **out /* ndev */);
int dsl_comm_destroy(dsl_comm *c);
/* ncclCommCount: how many ranks the communicator REALLY spans (a custom transport: the count it was created
 * with).  A bench or a host that asked for N ranks checks this instead of trusting its own arithmetic. */
int dsl_comm_count(dsl_comm *c, int *nranks);
const char *dsl_comm_last_error(void);
/* A communicator over the HOST'S OWN transport instead of RCCL (MPI, a socket layer, a test shim): the slab
 * drivers make exactly the same sequence of calls through this table as they make to RCCL (one group per
 * exchange: group_start, send per neighbour, recv per neighbour, group_end; all_reduce_max for the re-plan
 * words and the PCISPH iteration error).  Buffers are DEVICE pointers; `stream` is the hipStream_t the
 * operation is ordered on: it may start only once the work queued on that stream so far has finished, and
 * work queued on the stream after the call returns must see its result (RCCL's stream semantics; a blocking
 * implementation satisfies them by synchronising the stream first).  Inside a group nothing may block on
 * its peer before group_end.  Every callback returns 0 on success; the table is copied. */
typedef struct dsl_transport {
  void *ctx;
  int (*group_start)(void *ctx);
  int (*group_end)(void *ctx);
  int (*send)(void *ctx, const void *dev_buf, size_t bytes, int peer, void *stream);
  int (*recv)(void *ctx, void *dev_buf, size_t bytes, int peer, void *stream);
  int (*all_reduce_max_u32)(void *ctx, void *dev_buf /* in place */, size_t count, void *stream);
} dsl_transport;
int dsl_comm_create_custom(int nranks, int rank, int device, const dsl_transport *transport, dsl_comm **out);
int dsl_create_multi(const dsl_params *params /* ndev */, int ndev, const int *devices, dsl_handle **handles /* ndev */,
                     dsl_comm **comms /* ndev */);
int dsl_slab_attach(dsl_handle *h, dsl_comm *comm, int lo_rank, int hi_rank, float width_full, float width, int cap_full,
                    int cap_xonly, int overlap);
int dsl_slab_detach(dsl_handle *h);
/* periodic images along the slab axis: records arriving from the lower / upper neighbour are moved by
 * from_lo / from_hi (a ring of ranks closes with -L / +L at its two ends, 0 elsewhere) */
int dsl_slab_image_shift(dsl_handle *h, float from_lo, float from_hi);
int dsl_slab_exchange(dsl_handle *h);
int dsl_slab_replan(dsl_handle *h);
int dsl_slab_wcsph_step(dsl_handle *h, int nsteps);
int dsl_slab_pcisph_step(dsl_handle *h, int nsteps);
/* ---- multi-GPU: re-balancing by moving the slab planes during a run (opt-in) ----
 * A scene that is not symmetric along the slab axis leaves one rank with most of the particles.  Every M steps the
 * ranks count their owned particles per CELL LAYER along the axis (layer k = [origin + k edge, origin + (k+1) edge),
 * edge = the grid's cell edge, `origin` on a cell plane), sum the histograms, and every rank takes the same decision:
 * each interior plane moves ONE layer towards the layer boundary that splits the particles evenly.  The exchange that
 * exists carries the move: between an integrate and the pack that follows it every ghost is NaN, so ownership is purely
 * positional; whoever lies outside the new planes is packed as a migrant, and the old owner's 2h ghost band covers the
 * strip plus the neighbour's band for a move of up to 2h.  Off (the default) costs nothing: no kernel, no transport
 * call, the same bits.
 *
 * Building blocks, for a host that runs the exchange itself:
 * dsl_slab_layer_counts : overwrites dev_counts[0 .. n_layers) (DEVICE memory) with this handle's owned particles per
 *                      layer; coordinates outside [origin, origin + n_layers edge) count in the first / last layer.
 *                      Asynchronous.  DSL_ERR_INVALID without a slab, for n_layers outside [1, 4096], or if `origin`
 *                      is not on a cell plane of this handle's grid (1e-3 cell of slack).  When every live particle
 *                      has one owner and the planes are layer boundaries -- after an exchange -- the ranks' histograms
 *                      are disjoint, and a MAX all-reduce of them is their sum.
 * dsl_slab_move_planes : [lo, hi) of a configured slab changes, the particles are not touched; no host
 *                      synchronisation (unlike dsl_slab_config).  LEGAL ONLY BETWEEN AN INTEGRATE (dsl_force_pass,
 *                      DSL_PCI_END_STEP) AND THE NEXT dsl_slab_pack / dsl_slab_exchange, and by at most 2h per step;
 *                      the call cannot check that.  It refuses while a split force pass is pending (the band launch
 *                      integrated, and dsl_slab_pack_band would pack, the layers of the old planes: run that step
 *                      unsplit) and an empty range.
 * dsl_slab_get_planes  : the planes in force.  A host that classifies particles itself needs them once planes move.
 *
 * The native drivers (after dsl_slab_attach):
 * dsl_slab_rebalance   : every = M > 0 turns it on, 0 off (a move already planned is still applied).  `planes`
 *                      (nranks + 1 entries, in layers; [0] and [nranks] are the domain ends and never move) must be
 *                      this run's planes -- this rank's lo / hi equal origin + planes[rank] edge and origin +
 *                      planes[rank + 1] edge to 1e-3 cell, where they are finite --; plane r stays inside
 *                      [plane_min[r], plane_max[r]], and no slab gets thinner than min_layers (>= 2: the 2h band must
 *                      come from one neighbour).  [origin + plane_min edge - width, origin + plane_max edge + width]
 *                      of this rank's two planes must lie inside this handle's grid box, n_layers <= 4096: otherwise
 *                      DSL_ERR_INVALID, and dsl_last_error names the shortfall.  Identical arguments on every rank.
 *                      Then dsl_slab_wcsph_step / dsl_slab_pcisph_step LOOK after the exchange of every M-th step
 *                      (the count, ONE all_reduce_max_u32 over n_layers words, one host synchronisation, the plan) and
 *                      APPLY a plan that moves a plane in the next step, between its integrate and its pack; that one
 *                      step runs the unsplit exchange even with overlap = 1.  While it is on, the message re-plan adds
 *                      the fullest layer next to an interior plane (last histogram) to the full-record capacity: attach
 *                      with cap_full sized for the band plus one cell layer.  An undersized message or capacity remains
 *                      DSL_ERR_OVERFLOW on every rank at the next re-plan.
 * dsl_slab_rebalance_state : `planes` (nranks + 1): the last plan -- in force, but for a move the next step still has to
 *                      apply; `counts` (n_layers, or NULL): the last global histogram (zeros before the first look);
 *                      looks; plane moves planned so far.  Blocking. */
int dsl_slab_layer_counts(dsl_handle *h, float origin, int n_layers, int32_t *dev_counts);
int dsl_slab_move_planes(dsl_handle *h, float lo, float hi);
int dsl_slab_get_planes(dsl_handle *h, float *lo, float *hi);
int dsl_slab_rebalance(dsl_handle *h, int every, float origin, int n_layers, const int32_t *planes /* nranks + 1 */,
                       const int32_t *plane_min /* nranks + 1 */, const int32_t *plane_max /* nranks + 1 */, int min_layers);
int dsl_slab_rebalance_state(dsl_handle *h, int32_t *planes /* nranks + 1 */, int32_t *counts /* n_layers, or NULL */,
                             int64_t *looks, int64_t *moves);

/* Library options: behaviour that is the product's own and has no counterpart among the reference's parameters.
 *   DSL_OPT_SKIN (set/get): 0 = off, else a fraction s of h in (0, 0.2]; default 0.07 for DSL_MATH_FAST handles of at
 *       least 200,000 particles, 0 otherwise.  dsl_wcsph_step (DSL_MATH_FAST, grid
 *       neighbours, single domain, no boundary particles) then keeps one neighbour LIST per particle, built against the
 *       cut-off h (1 + s) on cells h (1 + s) wide, and walks it step after step until some particle may have moved
 *       s h / 2 since the build -- measured on the device, by the integrating kernel, against the build's reference
 *       positions (DSL_OPT_SKIN_PREDICT); only then does it sort and sweep again.  The sums are the reference's sums over { |x_i - x_j| < h }
 *       (sph_field.go:155-200,251-269): a listed pair beyond h contributes exactly 0.  The reference itself rebuilds
 *       its sampler only every 4th CacheIncr (fluid.go:208-215).  DSL_MATH_EXACT rebuilds every step.
 *       Once the flow outruns the skin (five of the last 16 steps rebuilt -- a rebuild costs about two steps), or more
 *       than one particle in 64 sits in a tile whose wider cells no longer fit the LDS image, the library suspends it by
 *       itself for the next 2048 steps (twice as long after every suspension in a row, up to 32768), then tries again; it looks every 32 steps, at step counts
 *       fixed in advance, so results never depend on timing.
 *   DSL_OPT_SKIN_STEPS / _REBUILDS / _LIST_OVERFLOW / _SUSPENSIONS (get): skin steps taken, how many of them rebuilt,
 *       whether some particle's list outgrew 95 entries (it then takes the global-memory sweep: correct, slow), how
 *       often the library suspended the skin. */
enum {
  DSL_OPT_SKIN = 1,
  DSL_OPT_SKIN_STEPS = 2,
  DSL_OPT_SKIN_REBUILDS = 3,
  DSL_OPT_SKIN_LIST_OVERFLOW = 4,
  DSL_OPT_SKIN_SUSPENSIONS = 5,
  DSL_OPT_DEVICE_BYTES = 6,       /* (get) device memory this handle has allocated so far */
  DSL_OPT_SKIN_FIELDS_OWN = 7,    /* (get, while skin steps are live) list fields the particles needed at the last rebuild ... */
  DSL_OPT_SKIN_FIELDS_PADDED = 8, /* ... and the fields their lists hold, padded to the longest list of each wave */
  DSL_OPT_SKIN_PREDICT = 9,       /* (set/get) in [0, 0.95], default 0.8: the lists are built at REFERENCE positions x + tau v --
                                     where a particle will be about half way through the lists' life -- and displacement is
                                     measured against those: the same budget s h / 2 then covers the way from -tau v to
                                     +tau v.  tau is chosen on the device at every rebuild so that the fastest particle
                                     uses this fraction of the budget at the build itself (at most 16 steps ahead); any
                                     reference is sound, the displacement test is the same.  0: built where the particles are */
  DSL_OPT_SKIN_TAU_STEPS = 10,    /* (get, while skin steps are live) tau of the last rebuild, in steps */
  /* the kernels' fall-back forms (A/B runs and tests; the defaults are the product).  Each is product code that some
   * configuration or failure path reaches, and tests/test_gpu_variants.py holds each to the default's parity bar. */
  DSL_OPT_DENSITY_PAIR = 16,      /* 1: FAST density sweep with two targets per lane (default); 0: one lane per target */
  DSL_OPT_CELL_KEYS = 17,         /* 1: in-cell ordering from per-cell key rows in the scatter pass itself; 0: two passes */
  DSL_OPT_TILE_BOX = 18,          /* tile-list enumeration boxes bx | by << 8 | bz << 16 (default 8,4,4); 0: linear order */
  DSL_OPT_PERSISTENT_BLOCKS = 19, /* cap on the persistent grids' workgroups (tests: few workgroups walk many tiles); 0: none */
  DSL_OPT_PCI_QTILED = 20,        /* binned DensityF: 1 LDS sweep over query tiles (default), 0 global-memory sweep */
  DSL_OPT_PCI_QPAIR = 21,         /* ... two queries of one cell per lane (default 1) */
  DSL_OPT_PCI_QROWS = 22,         /* ... per-cell query rows instead of a sorted array (default 1; 512 B per GRID CELL,
                                     allocated when the binned form is first used: 33 GB for the 64M scene's box) */
  DSL_OPT_LIST_BUILD = 24,        /* skin step: 1 the lists are built in lock step -- every lane of a wave produces one field per trip
                                     from a queue of its non-empty mask words (default); 0: one bit loop per mask word */
  DSL_OPT_GRID_OVERSUB = 25,      /* the tile kernels' grids are this many times the workgroups a chip holds at once (default 1:
                                     persistent workgroups, each walks its share of the tile list; k > 1: the hardware hands
                                     out k times as many, shorter shares as workgroups retire -- evens out tiles of unequal cost) */
  DSL_OPT_TILE_QUEUE = 26,        /* the two force kernels of a single domain draw their tiles from per-XCD counters as they go (a
                                     workgroup that drew cheap tiles takes more of them) instead of walking a share dealt in
                                     advance: 1 (default) from 8M particles on, 2 always, 0 never */
  DSL_OPT_PCI_QINCR = 23,         /* ... the rows kept from one correction iteration of a step to the next: only a query that
                                     has changed cells is moved (default 1; 0: every iteration fills the rows afresh) */
  DSL_OPT_COLLIDER_TRIANGLES = 32, /* (get) triangles of the collider mesh; 0: none */
  DSL_OPT_COLLIDE_HITS = 33,       /* (get, blocking) particles the last collide pass moved (counted by the kernel) */
  DSL_OPT_COLLIDE_CULL = 34,       /* (set/get, default 1) broad phase: a wave skips a triangle -- a chunk of 256 by its box -- that
                                      none of its particles can reach (csrc/kernels_collide.hpp states when); 0: every pair is
                                      tested.  Results are identical either way */
  /* A uniform-grid index over the collider's triangles (csrc/kernels_collide_index.hpp): a wave visits only the triangles
   * some lane of it could hit, in list order; results are the list walk's, bit for bit.  Built on the device (blocking)
   * inside dsl_collider_set_mesh while the option is on, and when option or edge change while a mesh is set; its memory is
   * counted in DSL_OPT_DEVICE_BYTES and freed with the mesh.  Budget: 2^22 cells, max(2^20, 64 T) list entries.  An edge
   * outside the budget, negative or non-finite is refused (DSL_ERR_INVALID; option, edge and index stay as they were --
   * from dsl_collider_set_mesh: the new mesh is set, without an index).  If the build fails on the device (DSL_ERR_NOMEM)
   * the mesh stays set, there is no index, and the list walk runs.  Used only while DSL_OPT_COLLIDE_CULL is 1. */
  DSL_OPT_COLLIDE_INDEX = 35,         /* (set/get, default 0) 0: the list walk; 1: the walk over the index */
  DSL_OPT_COLLIDE_INDEX_EDGE = 36,    /* (set/get) cell edge; 0 (default): the library's choice -- the mean extent of the regular
                                         triangles' padded boxes, doubled until the budget holds.  get: the edge in use, 0: no index */
  DSL_OPT_COLLIDE_INDEX_CELLS = 37,   /* (get) cells of the built index; 0: none */
  DSL_OPT_COLLIDE_INDEX_ENTRIES = 38, /* (get) cell-list entries plus always-list entries (the irregular triangles) */
  DSL_OPT_COLLIDE_VISITS = 39,        /* (get, blocking) triangle records loaded, summed over the waves of the last collide pass or
                                         query that the indexed kernel ran (full-walk waves included); -1: the list walk ran it */
  DSL_OPT_COLLIDE_FULL_WAVES = 40,    /* (get, blocking) waves of that launch that walked the whole list (a slow lane); -1 likewise */
  DSL_OPT_COLLIDE_SLAB = 41,          /* (set/get, default 0) 1: a collider mesh on a slab handle -- dsl_collider_set_mesh and
                                         dsl_slab_config accept each other, in either order; the rules are at dsl_collide_pass.
                                         Back to 0 while a slab handle holds a mesh: DSL_ERR_INVALID, nothing changes */
  /* dsl_field_volume.  1: DSL_MATH_FAST handles with grid neighbours sweep the lattice brick by brick (8 x 8 x 4 voxels
   * per workgroup) out of an LDS image of the particles in reach of the brick; a brick whose image does not fit takes the
   * per-voxel sweep over global memory.  0: the per-voxel sweep everywhere, bit for bit dsl_field_interpolate in both math
   * modes (DSL_MATH_EXACT and DSL_NEIGH_LSH_REF always run it).  Both forms give the same bits.  Default 1: at step = h / 2
   * the brick form is a quarter faster; at step >= h, where every brick inside the fluid falls back, it is a quarter slower
   * and 0 is the better choice (DESIGN.md 4.3 has the measurement). */
  DSL_OPT_VOLUME_BRICKS = 48,          /* (set/get, default 1) */
  DSL_OPT_VOLUME_LDS_BRICKS = 49,      /* (get, blocking) bricks of the last call that swept out of LDS; 0: the per-voxel form ran */
  DSL_OPT_VOLUME_FALLBACK_BRICKS = 50, /* (get, blocking) bricks of the last call whose image did not fit; 0 likewise */
  DSL_OPT_VOLUME_EMPTY_BRICKS = 51,    /* (get, blocking) bricks of the last call with no particle in reach: zeros, nothing staged */
  DSL_OPT_VOLUME_STAGED_RECORDS = 52,  /* (get, blocking) particle records (20 bytes each) the LDS bricks of the last call staged */
  /* dsl_surface_extract / dsl_field_surface, the last call's */
  DSL_OPT_SURFACE_TRIANGLES = 56,      /* (get, blocking) T, the full number of triangles */
  DSL_OPT_SURFACE_ACTIVE_BRICKS = 57,  /* (get, blocking) bricks of 8 x 8 x 4 cubes that emitted at least one triangle */
  DSL_OPT_SURFACE_COUNT_MS = 58,       /* (get, blocking) milliseconds of its count launch, from device events recorded while */
  DSL_OPT_SURFACE_SCAN_MS = 59,        /* dsl_timing_enable(1) holds (0 otherwise); its scan launches; */
  DSL_OPT_SURFACE_EMIT_MS = 60,        /* its emit launch (0 for a call that emitted nothing) */
  /* dsl_surface_extract_indexed / dsl_field_surface_indexed, the last call's */
  DSL_OPT_SURFACE_VERTICES = 61,           /* (get, blocking) V, the full number of vertices */
  DSL_OPT_SURFACE_MESH_VCOUNT_MS = 62,     /* (get, blocking) milliseconds of its vertex count launch, as DSL_OPT_SURFACE_COUNT_MS; */
  DSL_OPT_SURFACE_MESH_VSCAN_MS = 63,      /* its vertex scan launches; */
  DSL_OPT_SURFACE_MESH_VEMIT_MS = 64,      /* its vertex emit launch (0 for a call with cap_vertices = 0 or V = 0); */
  DSL_OPT_SURFACE_MESH_IEMIT_MS = 65,      /* its index emit launch (0 for a call with cap_triangles = 0 or without cubes) */
  /* dsl_mesh_distance_volume, the last call's */
  DSL_OPT_SDF_ACTIVE_BRICKS = 72,  /* (get, blocking) bricks of 8 x 8 x 4 voxels with a non-empty triangle list */
  DSL_OPT_SDF_VISITS = 73,         /* (get, blocking) triangle visits: (voxel, triangle) pairs the distance phase tested */
  DSL_OPT_SDF_DISTANCE_MS = 74,    /* (get, blocking) milliseconds of its distance launch, as DSL_OPT_SURFACE_COUNT_MS; */
  DSL_OPT_SDF_SIGN_MS = 75,        /* its sign launches: the marks' memset, the sweep, the parity (0 with DSL_SDF_UNSIGNED) */
  DSL_OPT_COLLIDER_VOLUME = 76,    /* (get) voxels of the volume collider; 0: none */
  DSL_OPT_COLLIDER_VOLUME_MOVING = 77,  /* (get) 1 while a motion is set */
  DSL_OPT_BODIES = 78,             /* (get) number of rigid bodies (dsl_body_add) */
  DSL_OPT_BODIES_INTEGRATE = 79,   /* (set/get, default 1) 0: the step drivers run the bodies' pass and fold but leave the
                                      poses alone -- a host that scripts all motion itself */
  DSL_OPT_BODIES_CONTACT = 80,     /* (set/get, default 0) bit 1: the bodies against the wall box, bit 2: against each other,
                                      behind each step's integration (dsl_contact_pass); other values: DSL_ERR_INVALID.  A
                                      list build that fails with DSL_ERR_NOMEM leaves the option as it was */
  DSL_OPT_BODIES_CONTACTS = 81,    /* (get, blocking) entries of the last solve that got past k > 0 */
  /* sources and sinks */
  DSL_OPT_EMITTERS = 88,           /* (get) number of emitters (dsl_emitter_add) */
  DSL_OPT_SINKS = 89,              /* (get) number of sinks (dsl_sink_add) */
  DSL_OPT_EMITTED = 90,            /* (get) particles emitted so far, by the step drivers and by dsl_emit */
  DSL_OPT_EMIT_SKIPPED = 91,       /* (get) layers the step drivers skipped because they did not fit the capacity */
  DSL_OPT_REMOVED = 92,            /* (get) particles the sinks removed so far */
  DSL_OPT_SINK_EVERY = 93,         /* (set/get, default 8) the step drivers apply the sinks at steps s with s % every == 0;
                                      0: only dsl_particles_remove does.  Negative or above 2^30: DSL_ERR_INVALID */
  /* the frame recorder (0 from all five while none is set) */
  DSL_OPT_RECORD_FRAMES = 96,      /* (get) frames recorded so far, by the step drivers and by dsl_record_now */
  DSL_OPT_RECORD_DROPPED = 97,     /* (get) frames dropped because no slot was released */
  DSL_OPT_RECORD_READY = 98,       /* (get) unreleased frames whose copy has landed (never blocks) */
  DSL_OPT_RECORD_PACK_MS = 99,     /* (get, blocking) milliseconds of the last frame's bounds + pack launches, as */
  DSL_OPT_RECORD_COPY_MS = 100     /* DSL_OPT_SURFACE_COUNT_MS; of the last frame's copy to its pinned slot */
};
int dsl_set_option(dsl_handle *h, int option, double value);
int dsl_get_option(dsl_handle *h, int option, double *value);

/* global particle ids of the current slots (host order of dsl_upload); default 0..n-1 */
int dsl_set_ids(dsl_handle *h, const int32_t *ids, size_t count);
/* Marks every force as equal to force_reset (the state Update leaves, fluid.go:193) */
int dsl_reset_forces(dsl_handle *h);

/* Error text of the last failing call on this handle (NULL handle: creation errors).
 * Replaces log.Fatalf in compute/gpu/gpu.go:52,66,234,339: the process is never aborted. */
const char *dsl_last_error(dsl_handle *h);
const char *dsl_version(void);

#ifdef __cplusplus
}
#endif
#endif
