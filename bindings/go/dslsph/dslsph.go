// Package dslsph is the cgo binding of libdslsph.so (include/dslsph.h), the MI355X
// SPH particle-step engine, shaped to drop in where dieselfluid's OpenCL path sits:
//
//	compute/gpu.ComputeGPU                  -> dslsph.ComputeGPU   (named float buffers)
//	solver/pcisph.GPUPredictorCorrector     -> dslsph.GPUPredictorCorrector
//	solver.SPHMethod (Run / Run_)           -> dslsph.WCSPH, dslsph.PCISPH
//
// NOT COMPILED IN THIS REPOSITORY'S CI: the build image has no Go toolchain (SURVEY.md
// section 0.2).  The file is deliberately thin and mechanical -- every method is one C call
// -- and the same call sequences are exercised from C++ (dieselfluid_amd/host) and Python
// (tests/) against the same library.  Build inside dieselfluid with
//
//	CGO_CFLAGS="-I<repo>/include" CGO_LDFLAGS="-L<repo>/dieselfluid_amd/lib -ldslsph" go build ./...
//
// cgo rules honoured: Go memory is only passed for the duration of a call (dsl_upload /
// dsl_download copy synchronously and retain nothing); the handle is an opaque C pointer;
// every library call re-selects its HIP device because goroutines migrate between OS
// threads.
package dslsph

/*
#cgo LDFLAGS: -ldslsph
#include <stdlib.h>
#include "dslsph.h"
*/
import "C"

import (
	"errors"
	"fmt"
	"io"
	"unsafe"
)

// Buffer names registered by New_GPUPredictorCorrector (solver/pcisph/pcisph_gpu_darwin.go:67-76).
var bufferIDs = map[string]C.int{
	"positions":  C.DSL_BUF_POSITIONS,
	"velocities": C.DSL_BUF_VELOCITIES,
	"forces":     C.DSL_BUF_FORCES,
	"densities":  C.DSL_BUF_DENSITIES,
	"pressures":  C.DSL_BUF_PRESSURES,
	"temps":      C.DSL_BUF_PCI_POSITIONS,
}

// parameter-block buffers of the reference that have no device array here
var auxBuffers = map[string]bool{"sizes": true, "floats": true, "sampler": true, "vecs": true}

// Engine owns one dsl_handle.
type Engine struct {
	h      *C.dsl_handle
	Params C.dsl_params
}

func lastError(h *C.dsl_handle) error { return errors.New(C.GoString(C.dsl_last_error(h))) }

// ReferenceParams returns sph.Init's constants for an n3^3 system (model/sph/fluid.go:41-88).
func ReferenceParams(n3 int) (C.dsl_params, error) {
	var p C.dsl_params
	if rc := C.dsl_params_reference(&p, C.int(n3)); rc != 0 {
		return p, lastError(nil)
	}
	return p, nil
}

// NewEngine replaces gpu.InitOpenCL + gpu.New_ComputeGPU (compute/gpu/gpu.go:45-119).
func NewEngine(p C.dsl_params, device int) (*Engine, error) {
	e := &Engine{Params: p}
	if rc := C.dsl_create(&e.Params, C.int(device), &e.h); rc != 0 {
		return nil, lastError(nil)
	}
	return e, nil
}

func (e *Engine) Close() {
	if e.h != nil {
		C.dsl_destroy(e.h)
		e.h = nil
	}
}

func (e *Engine) ck(rc C.int) error {
	if rc != 0 {
		return lastError(e.h)
	}
	return nil
}

// Upload / Download: ComputeGPU.PassFloatBuffer / ReadFloatBuffer (gpu.go:343-352,332-341).
func (e *Engine) Upload(buffer C.int, data []float32) error {
	if len(data) == 0 {
		return nil
	}
	return e.ck(C.dsl_upload(e.h, buffer, (*C.float)(unsafe.Pointer(&data[0])), C.size_t(len(data))))
}

func (e *Engine) Download(buffer C.int, data []float32) error {
	if len(data) == 0 {
		return nil
	}
	return e.ck(C.dsl_download(e.h, buffer, (*C.float)(unsafe.Pointer(&data[0])), C.size_t(len(data))))
}

// The passes of model/sph.SPH (model/sph/fluid.go:100-197), one C call each.
func (e *Engine) NN() error                    { return e.ck(C.dsl_build_neighbours(e.h)) }
func (e *Engine) DensityAll() error            { return e.ck(C.dsl_density_pass(e.h)) }
func (e *Engine) PressureAll() error           { return e.ck(C.dsl_pressure_pass(e.h)) }
func (e *Engine) ViscousAll() error            { return e.ck(C.dsl_viscous_pass(e.h)) }
func (e *Engine) GradientPressureForce() error { return e.ck(C.dsl_gradient_pressure_pass(e.h)) }
func (e *Engine) Update() error                { return e.ck(C.dsl_update_pass(e.h)) }
func (e *Engine) ExternalAll(f [3]float32) error {
	return e.ck(C.dsl_external_pass(e.h, (*C.float)(unsafe.Pointer(&f[0]))))
}
func (e *Engine) WCSPHStep(n int) error  { return e.ck(C.dsl_wcsph_step(e.h, C.int(n))) }
func (e *Engine) PCISPHBegin() error     { return e.ck(C.dsl_pcisph_begin(e.h)) }
func (e *Engine) PCISPHStep(n int) error { return e.ck(C.dsl_pcisph_step(e.h, C.int(n))) }
func (e *Engine) Sync() error            { return e.ck(C.dsl_sync(e.h)) }
func (e *Engine) SetParams() error       { return e.ck(C.dsl_set_params(e.h, &e.Params)) }

// ---- boundary particles (model/particle_array.go:123-128, model/field/sph_field.go:75-85) ----

// AddBoundaryParticles appends position-only particles behind the fluid (needs room in Params.capacity).
func (e *Engine) AddBoundaryParticles(positions []float32) error {
	if len(positions) == 0 {
		return nil
	}
	if err := e.ck(C.dsl_add_boundary_particles(e.h, (*C.float)(unsafe.Pointer(&positions[0])), C.size_t(len(positions)))); err != nil {
		return err
	}
	// the library's n_boundary has grown: refresh the copy that SetParams sends back and that sizes the buffers
	return e.ck(C.dsl_get_params(e.h, &e.Params))
}

// ---- the SPHField operators no solver calls (model/field/sph_field.go:124-135,203-294) ----

func (e *Engine) fieldOut(n int, call func(*C.float, C.size_t) C.int) ([]float32, error) {
	out := make([]float32, n)
	if n == 0 {
		return out, nil
	}
	return out, e.ck(call((*C.float)(unsafe.Pointer(&out[0])), C.size_t(n)))
}
func (e *Engine) Div(tensorBuffer C.int) ([]float32, error) {
	return e.fieldOut(int(e.Params.n_particles), func(p *C.float, n C.size_t) C.int { return C.dsl_field_divergence(e.h, tensorBuffer, p, n) })
}
func (e *Engine) Curl(tensorBuffer C.int) ([]float32, error) {
	return e.fieldOut(3*int(e.Params.n_particles), func(p *C.float, n C.size_t) C.int { return C.dsl_field_curl(e.h, tensorBuffer, p, n) })
}
func (e *Engine) Laplacian(scalarBuffer C.int) ([]float32, error) {
	return e.fieldOut(int(e.Params.n_particles), func(p *C.float, n C.size_t) C.int { return C.dsl_field_laplacian(e.h, scalarBuffer, p, n) })
}
func (e *Engine) Interpolate(scalarBuffer C.int, positions []float32) ([]float32, error) {
	out := make([]float32, len(positions)/3)
	if len(out) == 0 {
		return out, nil
	}
	return out, e.ck(C.dsl_field_interpolate(e.h, scalarBuffer, (*C.float)(unsafe.Pointer(&positions[0])), C.size_t(len(out)),
		(*C.float)(unsafe.Pointer(&out[0]))))
}

// InterpolateGrid: Interpolate at every point origin + step * (i, j, k) of a regular lattice (grid.Grid.GridPosition),
// x fastest: voxel (i, j, k) at (k*dims[1]+j)*dims[0]+i.  devOut (device memory, may be nil) is written asynchronously on
// the engine's stream; without it the values come back in a host slice.
func (e *Engine) InterpolateGrid(scalarBuffer C.int, origin, step [3]float32, dims [3]int32, devOut unsafe.Pointer) ([]float32, error) {
	var out []float32
	var host *C.float
	if devOut == nil {
		n := 1 // (dims the library refuses: one float, so that the refusal is the library's)
		if dims[0] >= 1 && dims[1] >= 1 && dims[2] >= 1 && int64(dims[0])*int64(dims[1])*int64(dims[2]) <= 1<<30 {
			n = int(dims[0]) * int(dims[1]) * int(dims[2])
		}
		out = make([]float32, n)
		host = (*C.float)(unsafe.Pointer(&out[0]))
	}
	return out, e.ck(C.dsl_field_volume(e.h, scalarBuffer, (*C.float)(unsafe.Pointer(&origin[0])), (*C.float)(unsafe.Pointer(&step[0])),
		(*C.int32_t)(unsafe.Pointer(&dims[0])), (*C.float)(devOut), host))
}

// SurfaceExtract: the iso-surface triangles of a device volume on InterpolateGrid's lattice (include/dslsph.h has the
// rule).  devVertices (9 floats per triangle) and devNormals (3, may be nil) take the first min(T, capTriangles) triangles,
// devCount (an int64 of device memory, may be nil) the full number T.  wantCount: T comes back too (a blocking 8-byte copy);
// without it the call is asynchronous on the engine's stream and returns -1.
func (e *Engine) SurfaceExtract(devVolume unsafe.Pointer, origin, step [3]float32, dims [3]int32, iso float32,
	devVertices, devNormals unsafe.Pointer, capTriangles int, devCount unsafe.Pointer, wantCount bool) (int64, error) {
	n := C.int64_t(-1)
	var hostCount *C.int64_t
	if wantCount {
		hostCount = &n
	}
	err := e.ck(C.dsl_surface_extract(e.h, (*C.float)(devVolume), (*C.float)(unsafe.Pointer(&origin[0])), (*C.float)(unsafe.Pointer(&step[0])),
		(*C.int32_t)(unsafe.Pointer(&dims[0])), C.float(iso), (*C.float)(devVertices), (*C.float)(devNormals),
		C.size_t(capTriangles), (*C.int64_t)(devCount), hostCount))
	return int64(n), err
}

// FieldSurface: InterpolateGrid and SurfaceExtract in one call, for a host without device memory: the first
// min(T, len(vertices)/9, len(normals)/3) triangles into vertices and, unless nil, normals (3 floats per triangle); returns T.
func (e *Engine) FieldSurface(scalarBuffer C.int, origin, step [3]float32, dims [3]int32, iso float32, vertices, normals []float32) (int64, error) {
	var n C.int64_t
	var vp, np *C.float
	capTriangles := len(vertices) / 9
	if len(vertices) > 0 {
		vp = (*C.float)(unsafe.Pointer(&vertices[0]))
	}
	if len(normals) > 0 {
		np = (*C.float)(unsafe.Pointer(&normals[0]))
		if len(normals)/3 < capTriangles { // (both slices take the same triangles)
			capTriangles = len(normals) / 3
		}
	}
	err := e.ck(C.dsl_field_surface(e.h, scalarBuffer, (*C.float)(unsafe.Pointer(&origin[0])), (*C.float)(unsafe.Pointer(&step[0])),
		(*C.int32_t)(unsafe.Pointer(&dims[0])), C.float(iso), vp, np, C.size_t(capTriangles), &n))
	return int64(n), err
}

// Surface: the fluid's iso-surface in mesh.Mesh order (geom/mesh/mesh.go:11-14): Vertexes as 3 * T points of 3 floats,
// Normals as T.  The buffer is sized from a guess (four triangles per voxel of the lattice's three faces) and FieldSurface is
// called a second time only when the guess was short.
func (e *Engine) Surface(scalarBuffer C.int, origin, step [3]float32, dims [3]int32, iso float32) (vertices, normals []float32, err error) {
	nx, ny, nz := int(dims[0]), int(dims[1]), int(dims[2])
	guess := 4 * (nx*ny + ny*nz + nz*nx)
	if guess < 1024 {
		guess = 1024
	}
	for try := 0; try < 2; try++ {
		vertices = make([]float32, 9*guess)
		normals = make([]float32, 3*guess)
		t, err := e.FieldSurface(scalarBuffer, origin, step, dims, iso, vertices, normals)
		if err != nil {
			return nil, nil, err
		}
		if int(t) <= guess {
			return vertices[:9*int(t)], normals[:3*int(t)], nil
		}
		guess = int(t)
	}
	return nil, nil, errors.New("dslsph: Surface: the triangle count changed between two calls")
}

// SurfaceExtractIndexed: the same surface as an indexed mesh (include/dslsph.h: dsl_surface_extract_indexed).  devPositions
// and devNormals (3 floats per vertex; devNormals may be nil) take the first min(V, capVertices) vertices, devIndices (3 int32
// per triangle) the first min(T, capTriangles) triples, devCounts (two int64 of device memory, may be nil) V and T.
// wantCounts: V and T come back too (a blocking copy); without it the call is asynchronous and returns -1, -1.  The mesh is
// complete only when both capacities suffice.
func (e *Engine) SurfaceExtractIndexed(devVolume unsafe.Pointer, origin, step [3]float32, dims [3]int32, iso float32,
	devPositions, devNormals unsafe.Pointer, capVertices int, devIndices unsafe.Pointer, capTriangles int,
	devCounts unsafe.Pointer, wantCounts bool) (int64, int64, error) {
	n := [2]C.int64_t{-1, -1}
	var hostCounts *C.int64_t
	if wantCounts {
		hostCounts = &n[0]
	}
	err := e.ck(C.dsl_surface_extract_indexed(e.h, (*C.float)(devVolume), (*C.float)(unsafe.Pointer(&origin[0])),
		(*C.float)(unsafe.Pointer(&step[0])), (*C.int32_t)(unsafe.Pointer(&dims[0])), C.float(iso), (*C.float)(devPositions),
		(*C.float)(devNormals), C.size_t(capVertices), (*C.int32_t)(devIndices), C.size_t(capTriangles), (*C.int64_t)(devCounts),
		hostCounts))
	return int64(n[0]), int64(n[1]), err
}

// FieldSurfaceIndexed: InterpolateGrid and SurfaceExtractIndexed in one call, for a host without device memory: the first
// min(V, len(positions)/3, len(normals)/3) vertices into positions and, unless nil, normals; the first min(T, len(indices)/3)
// triples into indices; returns V and T.
func (e *Engine) FieldSurfaceIndexed(scalarBuffer C.int, origin, step [3]float32, dims [3]int32, iso float32,
	positions, normals []float32, indices []int32) (int64, int64, error) {
	var n [2]C.int64_t
	var pp, np *C.float
	var ip *C.int32_t
	capVertices, capTriangles := len(positions)/3, len(indices)/3
	if len(positions) > 0 {
		pp = (*C.float)(unsafe.Pointer(&positions[0]))
	}
	if len(normals) > 0 {
		np = (*C.float)(unsafe.Pointer(&normals[0]))
		if len(normals)/3 < capVertices { // (both slices take the same vertices)
			capVertices = len(normals) / 3
		}
	}
	if len(indices) > 0 {
		ip = (*C.int32_t)(unsafe.Pointer(&indices[0]))
	}
	err := e.ck(C.dsl_field_surface_indexed(e.h, scalarBuffer, (*C.float)(unsafe.Pointer(&origin[0])), (*C.float)(unsafe.Pointer(&step[0])),
		(*C.int32_t)(unsafe.Pointer(&dims[0])), C.float(iso), pp, np, C.size_t(capVertices), ip, C.size_t(capTriangles), &n[0]))
	return int64(n[0]), int64(n[1]), err
}

// SurfaceIndexed: the fluid's iso-surface as positions, vertex normals (3 floats per vertex) and indices (3 per triangle).
// The buffers are sized from a guess (two vertices and four triangles per voxel of the lattice's three faces) and
// FieldSurfaceIndexed is called a second time only when a guess was short.
func (e *Engine) SurfaceIndexed(scalarBuffer C.int, origin, step [3]float32, dims [3]int32, iso float32) (positions, normals []float32, indices []int32, err error) {
	nx, ny, nz := int(dims[0]), int(dims[1]), int(dims[2])
	area := nx*ny + ny*nz + nz*nx
	capV, capT := 2*area, 4*area
	if capV < 1024 {
		capV = 1024
	}
	if capT < 1024 {
		capT = 1024
	}
	for try := 0; try < 2; try++ {
		positions = make([]float32, 3*capV)
		normals = make([]float32, 3*capV)
		indices = make([]int32, 3*capT)
		v, t, err := e.FieldSurfaceIndexed(scalarBuffer, origin, step, dims, iso, positions, normals, indices)
		if err != nil {
			return nil, nil, nil, err
		}
		if int(v) <= capV && int(t) <= capT {
			return positions[:3*int(v)], normals[:3*int(v)], indices[:3*int(t)], nil
		}
		if int(v) > capV {
			capV = int(v)
		}
		if int(t) > capT {
			capT = int(t)
		}
	}
	return nil, nil, nil, errors.New("dslsph: SurfaceIndexed: the counts changed between two calls")
}

// ---- render hand-off without the per-step full read-back (pcisph_gpu_darwin.go:276-282) ----

// DownloadDecimated: every stride-th particle of positions / velocities.
func (e *Engine) DownloadDecimated(buffer C.int, stride int, out []float32) error {
	if len(out) == 0 {
		return nil
	}
	return e.ck(C.dsl_download_decimated(e.h, buffer, C.int(stride), (*C.float)(unsafe.Pointer(&out[0])), C.size_t(len(out))))
}

// DevicePointers: the live SoA device arrays (x, y, z), the slot -> particle id map and the slot count.
func (e *Engine) DevicePointers(buffer C.int) (xyz [3]unsafe.Pointer, ids unsafe.Pointer, n int, err error) {
	var p [3]*C.float
	var i *C.int32_t
	var cn C.int
	err = e.ck(C.dsl_device_pointers(e.h, buffer, (**C.float)(unsafe.Pointer(&p[0])), &i, &cn))
	return [3]unsafe.Pointer{unsafe.Pointer(p[0]), unsafe.Pointer(p[1]), unsafe.Pointer(p[2])}, unsafe.Pointer(i), int(cn), err
}

// ---- lsh_ref parity mode (sampler/lsh/lsh.go) ----

func (e *Engine) SetHashVectors(vectors []float32) error { // lsh.Allocate's random projections, bits x 3
	return e.ck(C.dsl_set_hash_vectors(e.h, (*C.float)(unsafe.Pointer(&vectors[0])), C.int(len(vectors)/3)))
}

// ---- multi-GPU: one Engine per device, RCCL inside the library (include/dslsph.h) ----

// Comm wraps dsl_comm.  Rank 0 calls CommUniqueID and hands the 128 bytes to the other ranks over any channel.
type Comm struct{ c *C.dsl_comm }

func CommUniqueID() ([128]byte, error) {
	var id [128]byte
	if rc := C.dsl_comm_unique_id((*C.uint8_t)(unsafe.Pointer(&id[0]))); rc != 0 {
		return id, errors.New(C.GoString(C.dsl_comm_last_error()))
	}
	return id, nil
}
func NewComm(nranks, rank int, id [128]byte, device int) (*Comm, error) {
	c := &Comm{}
	if rc := C.dsl_comm_create(C.int(nranks), C.int(rank), (*C.uint8_t)(unsafe.Pointer(&id[0])), C.int(device), &c.c); rc != 0 {
		return nil, errors.New(C.GoString(C.dsl_comm_last_error()))
	}
	return c, nil
}
func (c *Comm) Close() { C.dsl_comm_destroy(c.c); c.c = nil }

// Count: the ranks the communicator really spans (ncclCommCount).
func (c *Comm) Count() (int, error) {
	var n C.int
	if rc := C.dsl_comm_count(c.c, &n); rc != 0 {
		return 0, errors.New(C.GoString(C.dsl_comm_last_error()))
	}
	return int(n), nil
}

// Transport: the host's own transport behind NewCommCustom (dsl_transport in include/dslsph.h).  The callbacks are C
// function pointers -- exported Go functions via //export, or plain C -- held as unsafe.Pointer so that packages other
// than this one can fill the table (cgo's C.dsl_transport is private to the package that imports "C").
type Transport struct {
	Ctx             unsafe.Pointer
	GroupStart      unsafe.Pointer // int (*)(void *ctx)
	GroupEnd        unsafe.Pointer // int (*)(void *ctx)
	Send            unsafe.Pointer // int (*)(void *ctx, const void *dev_buf, size_t bytes, int peer, void *stream)
	Recv            unsafe.Pointer // int (*)(void *ctx, void *dev_buf, size_t bytes, int peer, void *stream)
	AllReduceMaxU32 unsafe.Pointer // int (*)(void *ctx, void *dev_buf, size_t count, void *stream)
}

// NewCommCustom: a communicator over the host's own transport (MPI, sockets, ...) instead of RCCL.  The library calls
// the table's callbacks in exactly the order it would call RCCL; the table is copied.
func NewCommCustom(nranks, rank, device int, t Transport) (*Comm, error) {
	var table C.dsl_transport
	table.ctx = t.Ctx
	*(*unsafe.Pointer)(unsafe.Pointer(&table.group_start)) = t.GroupStart
	*(*unsafe.Pointer)(unsafe.Pointer(&table.group_end)) = t.GroupEnd
	*(*unsafe.Pointer)(unsafe.Pointer(&table.send)) = t.Send
	*(*unsafe.Pointer)(unsafe.Pointer(&table.recv)) = t.Recv
	*(*unsafe.Pointer)(unsafe.Pointer(&table.all_reduce_max_u32)) = t.AllReduceMaxU32
	c := &Comm{}
	if rc := C.dsl_comm_create_custom(C.int(nranks), C.int(rank), C.int(device), &table, &c.c); rc != 0 {
		return nil, errors.New(C.GoString(C.dsl_comm_last_error()))
	}
	return c, nil
}

// NewEngines: one process, several devices (dsl_create_multi: handles + ncclCommInitAll).  Drive each Engine
// from its own goroutine under runtime.LockOSThread: RCCL wants one host thread per device.
func NewEngines(params []C.dsl_params, devices []int) ([]*Engine, []*Comm, error) {
	n := len(devices)
	devs := make([]C.int, n)
	for k, d := range devices {
		devs[k] = C.int(d)
	}
	hs := make([]*C.dsl_handle, n)
	cs := make([]*C.dsl_comm, n)
	if rc := C.dsl_create_multi(&params[0], C.int(n), &devs[0], &hs[0], &cs[0]); rc != 0 {
		return nil, nil, lastError(nil)
	}
	engs, comms := make([]*Engine, n), make([]*Comm, n)
	for k := range hs {
		engs[k], comms[k] = &Engine{h: hs[k], Params: params[k]}, &Comm{c: cs[k]}
	}
	return engs, comms, nil
}

// SlabConfig / SlabAttach: this engine owns [lo, hi) along axis and exchanges a 2h band with the ranks lo_rank
// and hi_rank (-1 at a domain end) every step.
func (e *Engine) SlabConfig(axis int, lo, hi float32) error {
	return e.ck(C.dsl_slab_config(e.h, C.int(axis), C.float(lo), C.float(hi)))
}
func (e *Engine) SetIDs(ids []int32) error {
	return e.ck(C.dsl_set_ids(e.h, (*C.int32_t)(unsafe.Pointer(&ids[0])), C.size_t(len(ids))))
}
func (e *Engine) SlabAttach(c *Comm, loRank, hiRank int, widthFull, width float32, capFull, capX int, overlap bool) error {
	var cc *C.dsl_comm
	if c != nil {
		cc = c.c
	}
	ov := C.int(0)
	if overlap {
		ov = 1
	}
	return e.ck(C.dsl_slab_attach(e.h, cc, C.int(loRank), C.int(hiRank), C.float(widthFull), C.float(width), C.int(capFull), C.int(capX), ov))
}
func (e *Engine) SlabWCSPHStep(n int) error  { return e.ck(C.dsl_slab_wcsph_step(e.h, C.int(n))) }
func (e *Engine) SlabPCISPHStep(n int) error { return e.ck(C.dsl_slab_pcisph_step(e.h, C.int(n))) }
func (e *Engine) SlabReplan() error          { return e.ck(C.dsl_slab_replan(e.h)) }

// MaxV: SPH.MaxV() (fluid.go:206)
func (e *Engine) MaxV() (float32, error) {
	var st C.dsl_stats
	if err := e.ck(C.dsl_get_stats(e.h, &st)); err != nil {
		return 0, err
	}
	return float32(st.max_vel), nil
}

// ---------------------------------------------------------------------------------------
// compute/gpu.ComputeGPU facade (compute/gpu/gpu.go:20-425, compute/compute.go:26-53)
// ---------------------------------------------------------------------------------------

// Descriptor mirrors compute.Descriptor (compute/compute.go:9-13).
type Descriptor struct {
	Work  []int
	Local []int
	Size  int
}

type ComputeGPU struct {
	desc       *Descriptor
	eng        *Engine
	registered map[string]int
	kernels    map[string]bool
	pending    string
	log        string
}

func New_ComputeGPU(desc *Descriptor, eng *Engine) *ComputeGPU {
	return &ComputeGPU{desc: desc, eng: eng, registered: map[string]int{}, kernels: map[string]bool{}}
}

func (cp *ComputeGPU) RegisterBuffer(bytes_size int, t int, name string) error { // gpu.go:314-321
	if auxBuffers[name] {
		return nil
	}
	if _, ok := bufferIDs[name]; !ok {
		return fmt.Errorf("buffer [%s] is not a buffer of this engine", name)
	}
	cp.registered[name] = bytes_size
	return nil
}

func (cp *ComputeGPU) isregistered(name string) error { // gpu.go:305-310
	if _, ok := cp.registered[name]; !ok {
		return fmt.Errorf("buffer [%s] not registered", name)
	}
	return nil
}

func (cp *ComputeGPU) PassFloatBuffer(cpu_buffer []float32, name string) error { // gpu.go:343-352
	if auxBuffers[name] {
		return nil
	}
	if err := cp.isregistered(name); err != nil {
		return err
	}
	return cp.eng.Upload(bufferIDs[name], cpu_buffer)
}

func (cp *ComputeGPU) ReadFloatBuffer(cpu_buffer []float32, name string) error { // gpu.go:332-341
	if err := cp.isregistered(name); err != nil {
		return err
	}
	return cp.eng.Download(bufferIDs[name], cpu_buffer)
}

// PassLayoutBuffer (gpu.go:378-390) carries the two parameter blocks of pcisph_gpu_darwin.go:60-61.  They
// are not dropped: "sizes" {N, Nboundary, buckets, bucket_size} and "floats" {dt, mass, delta, maxVel, h}
// are checked against the engine's own parameters, so a host that disagrees with the device finds out.
func (cp *ComputeGPU) PassLayoutBuffer(data interface{}, bytes int, name string) error {
	if !auxBuffers[name] {
		return fmt.Errorf("buffer [%s] not registered", name)
	}
	p := &cp.eng.Params
	switch v := data.(type) {
	case []int32:
		if name == "sizes" && len(v) >= 2 && (C.int32_t(v[0]) != p.n_particles || C.int32_t(v[1]) != p.n_boundary) {
			return errors.New("sizes block {N, Nboundary, ..} does not match the engine's parameters")
		}
	case []float32:
		if name == "floats" && len(v) >= 5 && (C.float(v[0]) != p.dt || C.float(v[1]) != p.mass || C.float(v[4]) != p.h) {
			return errors.New("floats block {dt, mass, delta, maxVel, h} does not match the engine's parameters")
		}
	}
	cp.log += "Passed Layout Buffer " + name + "\n"
	return nil
}
func (cp *ComputeGPU) AddSourceFile(filename string) error   { return nil }  // gpu.go:257-271: nothing to compile
func (cp *ComputeGPU) AddSourceString(source string) bool    { return true } // compute.go:46
func (cp *ComputeGPU) BuildProgram(include_dir string) error { return nil }  // gpu.go:194-229

// ---- the rest of compute.GPUCompute (compute/compute.go:26-53) ----

// Setup (compute.go:29): the device context is the handle NewEngine made.
func (cp *ComputeGPU) Setup(gl bool) bool { return cp.HasDeviceContext() }

// Queue (gpu.go:286-296) names the built-in kernel the next Run executes.
func (cp *ComputeGPU) Queue(name string) error {
	if !cp.kernels[name] {
		return fmt.Errorf("kernel [%s] not registered", name)
	}
	cp.pending = name
	return nil
}

// Run (compute.go:33): the reference's two fused device kernels are phases of the PCISPH step here --
// compute_density (pci_density.c:12-23) = NN, density, viscosity; predict_correct (pci_predict.c:9-27) = the
// correction loop + integrate -- then THREAD_DONE (103) or THREAD_ERR (102) goes down the channel.
func (cp *ComputeGPU) Run(x chan int) {
	var rc C.int
	h := cp.eng.h
	switch cp.pending {
	case "compute_density":
		if rc = C.dsl_pcisph_begin(h); rc == 0 {
			rc = C.dsl_pcisph_phase(h, C.DSL_PCI_BEGIN_STEP)
		}
	case "predict_correct":
		for it := 0; rc == 0 && it < int(cp.eng.Params.pci_max_iters); it++ {
			if rc = C.dsl_pcisph_phase(h, C.DSL_PCI_ITERATE); rc == 0 {
				rc = C.dsl_pcisph_phase(h, C.DSL_PCI_CHECK)
			}
		}
		if rc == 0 {
			rc = C.dsl_pcisph_phase(h, C.DSL_PCI_END_STEP)
		}
	default:
		rc = C.DSL_ERR_INVALID
	}
	if rc == 0 {
		rc = C.dsl_sync(h)
	}
	if rc == 0 {
		x <- 103
	} else {
		x <- 102
	}
}

// PassIntBuffer / ReadIntBuffer (gpu.go:354-378): "sizes" is checked / returned; "sampler" (the host's
// flattened LSH table, lsh.go:70-80) is accepted and ignored on the way in -- the engine builds its own
// neighbour table -- and is HashSampler.GetData1D of the device table on the way out (DSL_NEIGH_LSH_REF).
func (cp *ComputeGPU) PassIntBuffer(cpu_buffer []int, name string) error {
	if !auxBuffers[name] {
		return cp.isregistered(name)
	}
	p := &cp.eng.Params
	if name == "sizes" && len(cpu_buffer) >= 2 && (C.int32_t(cpu_buffer[0]) != p.n_particles || C.int32_t(cpu_buffer[1]) != p.n_boundary) {
		return errors.New("sizes block {N, Nboundary, ..} does not match the engine's parameters")
	}
	cp.log += "Passed Integer Buffer " + name + "\n"
	return nil
}
func (cp *ComputeGPU) ReadIntBuffer(cpu_buffer []int, name string) error {
	p := &cp.eng.Params
	switch name {
	case "sizes":
		v := [4]int{int(p.n_particles), int(p.n_boundary), int(p.lsh_buckets), int(p.lsh_bucket_size)}
		copy(cpu_buffer, v[:])
		return nil
	case "sampler":
		t := make([]int32, len(cpu_buffer))
		if len(t) == 0 {
			return nil
		}
		if err := cp.eng.ck(C.dsl_lsh_download_table(cp.eng.h, (*C.int32_t)(unsafe.Pointer(&t[0])), C.size_t(len(t)))); err != nil {
			return err
		}
		for k := range t {
			cpu_buffer[k] = int(t[k])
		}
		return nil
	}
	return fmt.Errorf("buffer [%s] holds no integers", name)
}

// RegisterGLBuffer (gpu.go:323-330) shares a GL buffer with the device queue so that the renderer draws what
// the solver wrote without a read-back.  The counterpart here goes the other way: the consumer is handed the
// live device arrays (DevicePointers); the GL id is only recorded.
func (cp *ComputeGPU) RegisterGLBuffer(gl_buffer_id uint32, size int, name string) error {
	if name != "positions" {
		return errors.New("only the positions buffer has a render hand-off")
	}
	cp.registered[name] = size
	cp.log += fmt.Sprintf("RegisterGLBuffer() - buffer %s (GL id %d): read the device arrays through DevicePointers()\n", name, gl_buffer_id)
	return nil
}

func (cp *ComputeGPU) RegisterKernel(name string) bool { // gpu.go:231-250
	ok := name == "compute_density" || name == "predict_correct"
	if ok {
		cp.kernels[name] = true
	}
	return ok
}
func (cp *ComputeGPU) Set(d Descriptor)       { *cp.desc = d }
func (cp *ComputeGPU) Get() Descriptor        { return *cp.desc }
func (cp *ComputeGPU) HasDeviceContext() bool { return cp.eng != nil && cp.eng.h != nil }
func (cp *ComputeGPU) ValidState() bool       { return cp.HasDeviceContext() }
func (cp *ComputeGPU) Log() string            { return cp.log }

// ---- the rest of include/dslsph.h: one method per export, no logic -------------------------------------

func Version() string { return C.GoString(C.dsl_version()) }

func (e *Engine) GetParams() (C.dsl_params, error) {
	var p C.dsl_params
	err := e.ck(C.dsl_get_params(e.h, &p))
	return p, err
}
// Library options (DSL_OPT_* in include/dslsph.h) a host may want to name: the neighbour-list skin of WCSPHStep and its
// read-only counters, how far ahead of the particles the lists are built, the tile kernels' grid oversubscription.
const (
	OptSkin            = int(C.DSL_OPT_SKIN)
	OptSkinSteps       = int(C.DSL_OPT_SKIN_STEPS)
	OptSkinRebuilds    = int(C.DSL_OPT_SKIN_REBUILDS)
	OptSkinSuspensions = int(C.DSL_OPT_SKIN_SUSPENSIONS)
	OptSkinPredict     = int(C.DSL_OPT_SKIN_PREDICT)
	OptDeviceBytes     = int(C.DSL_OPT_DEVICE_BYTES)
	OptGridOversub     = int(C.DSL_OPT_GRID_OVERSUB)
	// the triangle-mesh collider: its size, the particles the last collide pass moved, the broad phase switch
	OptColliderTriangles = int(C.DSL_OPT_COLLIDER_TRIANGLES)
	OptCollideHits       = int(C.DSL_OPT_COLLIDE_HITS)
	OptCollideCull       = int(C.DSL_OPT_COLLIDE_CULL)
	// the cell index over the collider's triangles (include/dslsph.h)
	OptCollideIndex        = int(C.DSL_OPT_COLLIDE_INDEX)
	OptCollideIndexEdge    = int(C.DSL_OPT_COLLIDE_INDEX_EDGE)
	OptCollideIndexCells   = int(C.DSL_OPT_COLLIDE_INDEX_CELLS)
	OptCollideIndexEntries = int(C.DSL_OPT_COLLIDE_INDEX_ENTRIES)
	OptCollideVisits       = int(C.DSL_OPT_COLLIDE_VISITS)
	OptCollideFullWaves    = int(C.DSL_OPT_COLLIDE_FULL_WAVES)
	// a collider mesh on a slab handle: every rank sets the same mesh, the slab step drivers collide after each integrate
	OptCollideSlab = int(C.DSL_OPT_COLLIDE_SLAB)
	// the last SurfaceExtract / FieldSurface: its triangles T, its bricks of 8 x 8 x 4 cubes with a triangle
	OptSurfaceTriangles    = int(C.DSL_OPT_SURFACE_TRIANGLES)
	OptSurfaceActiveBricks = int(C.DSL_OPT_SURFACE_ACTIVE_BRICKS)
	// the last SurfaceExtractIndexed / FieldSurfaceIndexed: its vertices V
	OptSurfaceVertices = int(C.DSL_OPT_SURFACE_VERTICES)
)

// SetOption / GetOption: library options (DSL_OPT_* in include/dslsph.h), e.g. the neighbour-list skin of WCSPHStep.
func (e *Engine) SetOption(option int, value float64) error {
	return e.ck(C.dsl_set_option(e.h, C.int(option), C.double(value)))
}
func (e *Engine) GetOption(option int) (float64, error) {
	var v C.double
	err := e.ck(C.dsl_get_option(e.h, C.int(option), &v))
	return float64(v), err
}

func (e *Engine) ResetForces() error { return e.ck(C.dsl_reset_forces(e.h)) } // the state Update leaves (fluid.go:193)
func (e *Engine) ForcePass() error   { return e.ck(C.dsl_force_pass(e.h)) }   // fused [G] [V] X U of the WCSPH step

// SetStream: order the engine's launches on the caller's HIP stream (nil = the null stream); UseOwnStream undoes it.
func (e *Engine) SetStream(hipStream unsafe.Pointer) error { return e.ck(C.dsl_set_stream(e.h, hipStream)) }
func (e *Engine) UseOwnStream() error                      { return e.ck(C.dsl_use_own_stream(e.h)) }

// Count: live particles (owned + ghosts) and owned particles of a slab engine; blocking.
func (e *Engine) Count() (live, owned int, err error) {
	var a, b C.int
	err = e.ck(C.dsl_get_count(e.h, &a, &b))
	return int(a), int(b), err
}

// Per-kernel timing (HIP events on the launch stream): mode 0 off, 1 every kernel, 2 the dominant kernels only.
func (e *Engine) TimingEnable(mode int) error { return e.ck(C.dsl_timing_enable(e.h, C.int(mode))) }
func (e *Engine) TimingReset() error          { return e.ck(C.dsl_timing_reset(e.h)) }
func (e *Engine) Timing(kernelID int) (avgMs float64, launches int64, err error) {
	var ms C.double
	var n C.int64_t
	err = e.ck(C.dsl_timing_get(e.h, C.int(kernelID), &ms, &n))
	return float64(ms), int64(n), err
}

// Slot-order views (tests, debugging): a 3-component buffer without the un-sort, the slot -> particle id map,
// the cell table of the current neighbour build.
func (e *Engine) DownloadSorted(buffer C.int, out []float32) error {
	return e.ck(C.dsl_download_sorted(e.h, buffer, (*C.float)(unsafe.Pointer(&out[0])), C.size_t(len(out))))
}
func (e *Engine) DownloadIDs(out []int32) error {
	return e.ck(C.dsl_download_ids(e.h, (*C.int32_t)(unsafe.Pointer(&out[0])), C.size_t(len(out))))
}
func (e *Engine) DownloadCellStart(out []int32) error {
	return e.ck(C.dsl_download_cell_start(e.h, (*C.int32_t)(unsafe.Pointer(&out[0])), C.size_t(len(out))))
}

// Slab pieces for a host that brings its own transport (INTEGRATION.md 7b); device pointers are the caller's.
func SlabMessageFloats(capFull, capX int) int {
	return int(C.dsl_slab_message_floats(C.int(capFull), C.int(capX)))
}
func (e *Engine) SlabMessageFloats(capFull, capX int) int {
	return int(C.dsl_slab_message_floats_for(e.h, C.int(capFull), C.int(capX)))
}
func (e *Engine) SlabRecordFloats() int { return int(C.dsl_slab_record_floats(e.h)) }
func (e *Engine) SlabSplit(width, margin float32) error {
	return e.ck(C.dsl_slab_split(e.h, C.float(width), C.float(margin)))
}
func (e *Engine) ForcePassSplit(phase int) error { return e.ck(C.dsl_force_pass_split(e.h, C.int(phase))) }
func (e *Engine) SlabPack(widthFull, width float32, devLo, devHi unsafe.Pointer, capFull, capX int) error {
	return e.ck(C.dsl_slab_pack(e.h, C.float(widthFull), C.float(width), (*C.float)(devLo), (*C.float)(devHi), C.int(capFull), C.int(capX)))
}
func (e *Engine) SlabPackBand(widthFull float32, devLo, devHi unsafe.Pointer, capFull, capX int, stream unsafe.Pointer) error {
	return e.ck(C.dsl_slab_pack_band(e.h, C.float(widthFull), (*C.float)(devLo), (*C.float)(devHi), C.int(capFull), C.int(capX), stream))
}
func (e *Engine) SlabAppend(devMsg unsafe.Pointer, capFull, capX int) error {
	return e.ck(C.dsl_slab_append(e.h, (*C.float)(devMsg), C.int(capFull), C.int(capX)))
}
func (e *Engine) SlabAppend2(devMsgA, devMsgB unsafe.Pointer, capFull, capX int) error {
	return e.ck(C.dsl_slab_append2(e.h, (*C.float)(devMsgA), (*C.float)(devMsgB), C.int(capFull), C.int(capX)))
}

// SlabStatus: [0] records that did not fit, [1] split margin outrun, [2], [3] band high-water marks.
func (e *Engine) SlabStatus(resetHighWater bool) (st [4]int32, err error) {
	r := C.int(0)
	if resetHighWater {
		r = 1
	}
	err = e.ck(C.dsl_slab_status(e.h, (*C.int32_t)(unsafe.Pointer(&st[0])), r))
	return st, err
}
func (e *Engine) SlabOverflow() (highWater int, err error) {
	var hw C.int
	err = e.ck(C.dsl_slab_overflow(e.h, &hw))
	return int(hw), err
}
func (e *Engine) SlabDetach() error   { return e.ck(C.dsl_slab_detach(e.h)) }
func (e *Engine) SlabExchange() error { return e.ck(C.dsl_slab_exchange(e.h)) }

// SlabImageShift: periodic images along the slab axis (a ring of ranks closes with -L / +L at its two ends).
func (e *Engine) SlabImageShift(fromLo, fromHi float32) error {
	return e.ck(C.dsl_slab_image_shift(e.h, C.float(fromLo), C.float(fromHi)))
}

// Re-balancing: the slab planes move during a run (include/dslsph.h; DESIGN.md 6).  SlabRebalance hands it to the native
// step drivers: every = M > 0 steps between looks, 0 = off; planes and their bounds in cell layers from origin, one entry
// per rank plus one, identical on every rank.
func (e *Engine) SlabRebalance(every int, origin float32, nLayers int, planes, planeMin, planeMax []int32, minLayers int) error {
	var p, lo, hi *C.int32_t
	if every > 0 {
		if len(planes) < 2 || len(planeMin) != len(planes) || len(planeMax) != len(planes) {
			return errors.New("dslsph: SlabRebalance wants planes, planeMin and planeMax of ranks + 1 entries each")
		}
		p, lo, hi = (*C.int32_t)(unsafe.Pointer(&planes[0])), (*C.int32_t)(unsafe.Pointer(&planeMin[0])), (*C.int32_t)(unsafe.Pointer(&planeMax[0]))
	}
	return e.ck(C.dsl_slab_rebalance(e.h, C.int(every), C.float(origin), C.int(nLayers), p, lo, hi, C.int(minLayers)))
}

// SlabRebalanceState: the planes of the last plan (ranks + 1), the last global histogram (nLayers), looks and plane moves
// so far.  Blocking.
func (e *Engine) SlabRebalanceState(ranks, nLayers int) (planes, counts []int32, looks, moves int64, err error) {
	planes, counts = make([]int32, ranks+1), make([]int32, nLayers)
	var l, m C.int64_t
	var cp *C.int32_t
	if nLayers > 0 {
		cp = (*C.int32_t)(unsafe.Pointer(&counts[0]))
	}
	err = e.ck(C.dsl_slab_rebalance_state(e.h, (*C.int32_t)(unsafe.Pointer(&planes[0])), cp, &l, &m))
	return planes, counts, int64(l), int64(m), err
}

// SlabPlanes: the planes in force (a host that classifies particles itself needs them once planes move).
func (e *Engine) SlabPlanes() (lo, hi float32, err error) {
	var l, h C.float
	err = e.ck(C.dsl_slab_get_planes(e.h, &l, &h))
	return float32(l), float32(h), err
}

// The building blocks, for a host that runs the exchange itself: owned particles per cell layer into nLayers int32 words of
// device memory (asynchronous), and new planes without touching the particles -- legal only between an integrate and the next
// pack.
func (e *Engine) SlabLayerCounts(origin float32, nLayers int, devCounts unsafe.Pointer) error {
	return e.ck(C.dsl_slab_layer_counts(e.h, C.float(origin), C.int(nLayers), (*C.int32_t)(devCounts)))
}
func (e *Engine) SlabMovePlanes(lo, hi float32) error {
	return e.ck(C.dsl_slab_move_planes(e.h, C.float(lo), C.float(hi)))
}

// PCISPHErrorWord: copy the iteration's max density error out to / back in from a device word of the caller's
// (the all-reduce between DSL_PCI_ITERATE and DSL_PCI_CHECK of a host-driven slab step).
func (e *Engine) PCISPHErrorWord(devWord unsafe.Pointer, store bool) error {
	s := C.int(0)
	if store {
		s = 1
	}
	return e.ck(C.dsl_pcisph_error_word(e.h, (*C.uint32_t)(devWord), s))
}

// PCISPHSetBinning: -1 never, 0 automatic (default), 1 always -- whether the DensityF query points (the predictor's
// positions, which the reference never re-synchronises: pcisph_darwin.go:28-41) are sorted into grid cells of their own.
func (e *Engine) PCISPHSetBinning(mode int) error {
	return e.ck(C.dsl_pcisph_set_binning(e.h, C.int(mode)))
}

// PCISPHBinning: the mode, and whether the next correction iteration will sort its queries.
func (e *Engine) PCISPHBinning() (mode int, active bool, err error) {
	var m, a C.int
	err = e.ck(C.dsl_pcisph_get_binning(e.h, &m, &a, nil))
	return int(m), a != 0, err
}

// PCISPHQueryEscaped (slab mode, blocking): a query point of an owned particle has drifted more than h beyond a slab
// plane, out of what the 2h ghost band covers.
func (e *Engine) PCISPHQueryEscaped() (bool, error) {
	var x C.int
	err := e.ck(C.dsl_pcisph_get_binning(e.h, nil, nil, &x))
	return x != 0, err
}

// NewCommAll: one process, several devices (ncclCommInitAll); NewEngines wraps it together with the handles.
func NewCommAll(devices []int) ([]*Comm, error) {
	n := len(devices)
	devs := make([]C.int, n)
	for k, d := range devices {
		devs[k] = C.int(d)
	}
	cs := make([]*C.dsl_comm, n)
	if rc := C.dsl_comm_create_all(C.int(n), &devs[0], &cs[0]); rc != 0 {
		return nil, errors.New(C.GoString(C.dsl_comm_last_error()))
	}
	out := make([]*Comm, n)
	for k := range cs {
		out[k] = &Comm{c: cs[k]}
	}
	return out, nil
}

// ---- geom.Collider on the device: Mesh.Collision (geom/mesh/mesh.go:41-57) for every fluid particle ----

// SetColliderMesh hands T triangles (9 vertex floats and 3 normal floats each, in list order; the normals are used as
// supplied) to the device; an empty list removes the collider.  While a mesh is set WCSPHStep and PCISPHStep run the
// collide pass after Update.
func (e *Engine) SetColliderMesh(vertices, normals []float32, radius, restitution float32) error {
	if len(normals)%3 != 0 || len(vertices) != 3*len(normals) {
		return errors.New("SetColliderMesh: 9 vertex floats and 3 normal floats per triangle")
	}
	if len(normals) == 0 {
		return e.ck(C.dsl_collider_set_mesh(e.h, nil, nil, 0, C.float(radius), C.float(restitution)))
	}
	return e.ck(C.dsl_collider_set_mesh(e.h, (*C.float)(unsafe.Pointer(&vertices[0])), (*C.float)(unsafe.Pointer(&normals[0])), C.size_t(len(normals)/3), C.float(radius), C.float(restitution)))
}

// CollidePass: query + response for every fluid particle (asynchronous).
func (e *Engine) CollidePass() error { return e.ck(C.dsl_collide_pass(e.h)) }

// ColliderQuery: Mesh.Collision's returns for every fluid particle in host order, no response (blocking): the colliding
// triangle's index or -1, its normal, the barycentric coordinates, the rewound position.
func (e *Engine) ColliderQuery() (tri []int32, normal, coord, point []float32, err error) {
	n := int(e.Params.n_particles)
	tri = make([]int32, n)
	normal, coord, point = make([]float32, 3*n), make([]float32, 3*n), make([]float32, 3*n)
	err = e.ColliderQueryInto(tri, normal, coord, point)
	return
}

// ColliderQueryInto: ColliderQuery into the caller's slices (N, 3N, 3N, 3N long); a nil slice is a result the caller
// does not want: it is neither computed into a buffer nor downloaded (the C call's NULL pointer).
func (e *Engine) ColliderQueryInto(tri []int32, normal, coord, point []float32) error {
	n := int(e.Params.n_particles)
	if (tri != nil && len(tri) != n) || (normal != nil && len(normal) != 3*n) || (coord != nil && len(coord) != 3*n) || (point != nil && len(point) != 3*n) {
		return errors.New("ColliderQueryInto: tri holds N, normal, coord and point 3 N values (or are nil)")
	}
	fp := func(s []float32) *C.float {
		if len(s) == 0 {
			return nil
		}
		return (*C.float)(unsafe.Pointer(&s[0]))
	}
	var tp *C.int32_t
	if len(tri) != 0 {
		tp = (*C.int32_t)(unsafe.Pointer(&tri[0]))
	}
	return e.ck(C.dsl_collider_query(e.h, tp, fp(normal), fp(coord), fp(point)))
}

// ---- implicit colliders: the distance volume of a mesh, collision against a distance volume (include/dslsph.h) ----

const (
	// flags of MeshDistanceVolume and SetColliderVolume: distances without a sign (an open mesh, a thin shell)
	SdfUnsigned = int(C.DSL_SDF_UNSIGNED)
	// the timing id of MeshDistanceVolume's launches (dsl_timing_get)
	KSdf = int(C.DSL_K_SDF)
	// the last MeshDistanceVolume: its bricks of 8 x 8 x 4 voxels with a triangle list, the (voxel, triangle) pairs tested,
	// the milliseconds of its distance and sign phases (while timing is on); the voxels of the volume collider (0: none)
	OptSdfActiveBricks = int(C.DSL_OPT_SDF_ACTIVE_BRICKS)
	OptSdfVisits       = int(C.DSL_OPT_SDF_VISITS)
	OptSdfDistanceMs   = int(C.DSL_OPT_SDF_DISTANCE_MS)
	OptSdfSignMs       = int(C.DSL_OPT_SDF_SIGN_MS)
	OptColliderVolume  = int(C.DSL_OPT_COLLIDER_VOLUME)
)

// MeshDistanceVolume: the signed distance (negative inside; flags = SdfUnsigned: no sign) of every point of the lattice
// origin + step * (i, j, k) to the triangles (9 floats each), cut off at band (+Inf: no cut), x fastest.  devOut (device
// memory, dims[0]*dims[1]*dims[2] floats, written on the engine's stream) and hostOut (as many floats, blocking) may each
// be nil, not both.
func (e *Engine) MeshDistanceVolume(vertices []float32, origin, step [3]float32, dims [3]int32, band float32, flags int, devOut unsafe.Pointer, hostOut []float32) error {
	if len(vertices) == 0 || len(vertices)%9 != 0 {
		return errors.New("MeshDistanceVolume: 9 vertex floats per triangle, at least one triangle")
	}
	var hp *C.float
	if len(hostOut) > 0 {
		if len(hostOut) < int(dims[0])*int(dims[1])*int(dims[2]) {
			return errors.New("MeshDistanceVolume: hostOut is shorter than the lattice")
		}
		hp = (*C.float)(unsafe.Pointer(&hostOut[0]))
	}
	return e.ck(C.dsl_mesh_distance_volume(e.h, (*C.float)(unsafe.Pointer(&vertices[0])), C.size_t(len(vertices)/9), (*C.float)(unsafe.Pointer(&origin[0])), (*C.float)(unsafe.Pointer(&step[0])), (*C.int32_t)(unsafe.Pointer(&dims[0])), C.float(band), C.int(flags), (*C.float)(devOut), hp))
}

// SetColliderVolume: a distance volume as the collider of the step -- devVolume (device memory) or hostVolume, exactly one
// of them; the library keeps a copy.  A particle closer than radius to the surface is pushed out along the volume's
// gradient and reflected.  It excludes a collider mesh.  RemoveColliderVolume removes it.
func (e *Engine) SetColliderVolume(devVolume unsafe.Pointer, hostVolume []float32, origin, step [3]float32, dims [3]int32, radius, restitution float32, flags int) error {
	var hp *C.float
	if len(hostVolume) > 0 {
		if len(hostVolume) < int(dims[0])*int(dims[1])*int(dims[2]) {
			return errors.New("SetColliderVolume: hostVolume is shorter than the lattice")
		}
		hp = (*C.float)(unsafe.Pointer(&hostVolume[0]))
	}
	return e.ck(C.dsl_collider_set_volume(e.h, (*C.float)(devVolume), hp, (*C.float)(unsafe.Pointer(&origin[0])), (*C.float)(unsafe.Pointer(&step[0])), (*C.int32_t)(unsafe.Pointer(&dims[0])), C.float(radius), C.float(restitution), C.int(flags)))
}

func (e *Engine) RemoveColliderVolume() error {
	return e.ck(C.dsl_collider_set_volume(e.h, nil, nil, nil, nil, nil, 0, 0, 0))
}

// ColliderVolumeQuery: the interpolated distance (N) and the unit gradient (3 N) of the volume collider at every fluid
// particle in host order, no response (blocking); zeros where a particle lies in no cell of the volume.
func (e *Engine) ColliderVolumeQuery() (dist, normal []float32, err error) {
	n := int(e.Params.n_particles)
	dist, normal = make([]float32, n), make([]float32, 3*n)
	if n == 0 {
		return
	}
	err = e.ck(C.dsl_collider_volume_query(e.h, (*C.float)(unsafe.Pointer(&dist[0])), (*C.float)(unsafe.Pointer(&normal[0]))))
	return
}

// ---- the volume collider in rigid motion (include/dslsph.h: dsl_collider_volume_motion) ----

// 1 while a motion is set (dsl_get_option)
const OptColliderVolumeMoving = int(C.DSL_OPT_COLLIDER_VOLUME_MOVING)

// ColliderMotion: the rigid motion of the volume collider -- the reference's Collider.Origin / UpdateOrigin
// (render/mesh/collider.go:10-36) with an orientation and the body's velocities.  Rot: row-major R, its columns the body's
// axes in world coordinates; Trans: the body frame's origin; LinVel: the body's velocity there; AngVel: its angular
// velocity; all in world coordinates.
type ColliderMotion struct {
	Rot    [9]float32
	Trans  [3]float32
	LinVel [3]float32
	AngVel [3]float32
}

// IdentityMotion: the body where it was built, at rest
func IdentityMotion() ColliderMotion {
	return ColliderMotion{Rot: [9]float32{1, 0, 0, 0, 1, 0, 0, 0, 1}}
}

// SetColliderVolumeMotion: the pose and velocities every later collide pass uses; the voxels are not touched, nothing is
// synchronised.  The library does not integrate the pose: a host that moves a body calls this between single steps.
func (e *Engine) SetColliderVolumeMotion(m ColliderMotion) error {
	return e.ck(C.dsl_collider_volume_motion(e.h, (*C.float)(unsafe.Pointer(&m.Rot[0])), (*C.float)(unsafe.Pointer(&m.Trans[0])), (*C.float)(unsafe.Pointer(&m.LinVel[0])), (*C.float)(unsafe.Pointer(&m.AngVel[0]))))
}

// ClearColliderVolumeMotion: motion off (Collider.IsStatic again): the static pass runs
func (e *Engine) ClearColliderVolumeMotion() error {
	return e.ck(C.dsl_collider_volume_motion(e.h, nil, nil, nil, nil))
}

// ColliderVolumeImpulse: what the fluid handed to the body since the last reset -- the impulse and the torque impulse about
// Trans (blocking); reset zeroes the accumulators after the read.
func (e *Engine) ColliderVolumeImpulse(reset bool) (impulse, torque [3]float32, err error) {
	r := 0
	if reset {
		r = 1
	}
	err = e.ck(C.dsl_collider_volume_impulse(e.h, (*C.float)(unsafe.Pointer(&impulse[0])), (*C.float)(unsafe.Pointer(&torque[0])), C.int(r)))
	return
}

// ---- rigid bodies: several volume colliders, their poses integrated on the device (include/dslsph.h: dsl_body_add) ----

const (
	// the most bodies a handle takes
	MaxBodies = int(C.DSL_MAX_BODIES)
	// the number of bodies (get); 1: the step drivers integrate the poses (set/get, default 1)
	OptBodies          = int(C.DSL_OPT_BODIES)
	OptBodiesIntegrate = int(C.DSL_OPT_BODIES_INTEGRATE)
)

// BodyProps: the inverse mass, the inverse principal moments about the axes of the body's frame, a constant acceleration
// (gravity), and the collider's radius and restitution.  InvMass, InvInertia and Accel all zero: a kinematic body.
type BodyProps struct {
	InvMass     float32
	InvInertia  [3]float32
	Accel       [3]float32
	Radius      float32
	Restitution float32
}

// BodyState: the orientation Quat (w, x, y, z), the body frame's origin Trans in world coordinates (the point torques
// refer to: the centre of mass), its velocity LinVel and the angular velocity AngVel, world.
type BodyState struct {
	Quat   [4]float32
	Trans  [3]float32
	LinVel [3]float32
	AngVel [3]float32
}

// BodyAtRest: the identity, at rest
func BodyAtRest() BodyState {
	return BodyState{Quat: [4]float32{1, 0, 0, 0}}
}

func (p *BodyProps) c() C.dsl_body_props {
	var out C.dsl_body_props
	out.inv_mass = C.float(p.InvMass)
	for a := 0; a < 3; a++ {
		out.inv_inertia[a] = C.float(p.InvInertia[a])
		out.accel[a] = C.float(p.Accel[a])
	}
	out.radius = C.float(p.Radius)
	out.restitution = C.float(p.Restitution)
	return out
}

func (s *BodyState) c() C.dsl_body_state {
	var out C.dsl_body_state
	for a := 0; a < 4; a++ {
		out.quat[a] = C.float(s.Quat[a])
	}
	for a := 0; a < 3; a++ {
		out.trans[a] = C.float(s.Trans[a])
		out.lin_vel[a] = C.float(s.LinVel[a])
		out.ang_vel[a] = C.float(s.AngVel[a])
	}
	return out
}

// AddBody: a rigid body from a distance volume -- devVolume (device memory) or hostVolume, exactly one of them; the
// library keeps a copy.  Bodies get the ids 0, 1, ... in the order they were added, which is the order the pass applies
// them in.  It excludes a collider mesh and the single volume collider.
func (e *Engine) AddBody(devVolume unsafe.Pointer, hostVolume []float32, origin, step [3]float32, dims [3]int32, props BodyProps, state BodyState) (id int, err error) {
	var hp *C.float
	if len(hostVolume) > 0 {
		if len(hostVolume) < int(dims[0])*int(dims[1])*int(dims[2]) {
			return -1, errors.New("AddBody: hostVolume is shorter than the lattice")
		}
		hp = (*C.float)(unsafe.Pointer(&hostVolume[0]))
	}
	cp, cs := props.c(), state.c()
	var cid C.int
	err = e.ck(C.dsl_body_add(e.h, (*C.float)(devVolume), hp, (*C.float)(unsafe.Pointer(&origin[0])), (*C.float)(unsafe.Pointer(&step[0])), (*C.int32_t)(unsafe.Pointer(&dims[0])), &cp, &cs, &cid))
	return int(cid), err
}

// ClearBodies: removes every body (there is no removal of one: the order is part of the rule)
func (e *Engine) ClearBodies() error {
	return e.ck(C.dsl_bodies_clear(e.h))
}

// SetBodyState, SetBodyProps: between steps; they hold from the next pass on
func (e *Engine) SetBodyState(body int, state BodyState) error {
	cs := state.c()
	return e.ck(C.dsl_body_set_state(e.h, C.int(body), &cs))
}

func (e *Engine) SetBodyProps(body int, props BodyProps) error {
	cp := props.c()
	return e.ck(C.dsl_body_set_props(e.h, C.int(body), &cp))
}

// BodyState: the state the device holds and what the fluid handed to the body since the last reset -- the impulse and
// the torque impulse about Trans (blocking); reset zeroes the accumulators after the read.
func (e *Engine) BodyState(body int, reset bool) (state BodyState, impulse, torque [3]float32, err error) {
	r := 0
	if reset {
		r = 1
	}
	var cs C.dsl_body_state
	err = e.ck(C.dsl_body_get_state(e.h, C.int(body), &cs, (*C.float)(unsafe.Pointer(&impulse[0])), (*C.float)(unsafe.Pointer(&torque[0])), C.int(r)))
	for a := 0; a < 4; a++ {
		state.Quat[a] = float32(cs.quat[a])
	}
	for a := 0; a < 3; a++ {
		state.Trans[a] = float32(cs.trans[a])
		state.LinVel[a] = float32(cs.lin_vel[a])
		state.AngVel[a] = float32(cs.ang_vel[a])
	}
	return
}

// BodyQuery: the interpolated distance (N) and the world-space unit gradient (3 N) of one body at its current pose, at
// every fluid particle in host order, no response (blocking).
func (e *Engine) BodyQuery(body int) (dist, normal []float32, err error) {
	n := int(e.Params.n_particles)
	dist, normal = make([]float32, n), make([]float32, 3*n)
	if n == 0 {
		return
	}
	err = e.ck(C.dsl_body_query(e.h, C.int(body), (*C.float)(unsafe.Pointer(&dist[0])), (*C.float)(unsafe.Pointer(&normal[0]))))
	return
}

// ---- the bodies' contact stage: the wall box and each other (include/dslsph.h: dsl_contact_points) ----

const (
	// bit 1: walls, bit 2: bodies -- the step drivers detect and solve behind each integration (set/get, default 0);
	// the entries of the last solve that got past k > 0 (get, blocking)
	OptBodiesContact  = int(C.DSL_OPT_BODIES_CONTACT)
	OptBodiesContacts = int(C.DSL_OPT_BODIES_CONTACTS)
	ContactWalls      = 1
	ContactBodies     = 2
)

// ContactPoints: the voxel indices of a body's contact points, ascending (blocking)
func (e *Engine) ContactPoints(body int) (voxels []int32, err error) {
	var m C.int64_t
	if err = e.ck(C.dsl_contact_points(e.h, C.int(body), nil, 0, &m)); err != nil || m == 0 {
		return
	}
	voxels = make([]int32, int(m))
	err = e.ck(C.dsl_contact_points(e.h, C.int(body), (*C.int32_t)(unsafe.Pointer(&voxels[0])), C.size_t(len(voxels)), &m))
	return
}

// ContactPass: detection at the current poses for kinds, whatever the option is, and the solve behind it if asked
func (e *Engine) ContactPass(kinds int, solve bool) error {
	s := 0
	if solve {
		s = 1
	}
	return e.ck(C.dsl_contact_pass(e.h, C.int(kinds), C.int(s)))
}

// ContactTable: E of the last detection over k bodies, [body][target][9] = S (3), N (3), W, C, D (blocking)
func (e *Engine) ContactTable(k int) (table []float32, err error) {
	table = make([]float32, 9*k*(6+k))
	if len(table) == 0 {
		return
	}
	err = e.ck(C.dsl_contact_table(e.h, (*C.float)(unsafe.Pointer(&table[0])), C.size_t(len(table))))
	return
}

// ---- sources and sinks: fluid emitted and removed on the device (include/dslsph.h: dsl_particles_append) ----

const (
	MaxEmitters = int(C.DSL_MAX_EMITTERS)
	MaxSinks    = int(C.DSL_MAX_SINKS)
	// the timing id of the emit launch, the sink count and the compaction's launches (dsl_timing_get)
	KSources = int(C.DSL_K_SOURCES)
	// emitters and sinks in place; particles emitted, layers skipped for want of room, particles removed (all get);
	// the step drivers apply the sinks at steps s with s % every == 0 (set/get, default 8; 0: only RemoveParticles does)
	OptEmitters    = int(C.DSL_OPT_EMITTERS)
	OptSinks       = int(C.DSL_OPT_SINKS)
	OptEmitted     = int(C.DSL_OPT_EMITTED)
	OptEmitSkipped = int(C.DSL_OPT_EMIT_SKIPPED)
	OptRemoved     = int(C.DSL_OPT_REMOVED)
	OptSinkEvery   = int(C.DSL_OPT_SINK_EVERY)
)

// Emitter: lattice point (a, b) of the face lies at Origin + a U + b V; a layer every Period-th step from FirstStep on
type Emitter struct {
	Origin, U, V, Velocity [3]float32
	Nu, Nv                 int
	Ellipse                bool
	Period                 int
	FirstStep, MaxLayers   int64
}

// Sink: particles inside [Min, Max) go (Outside: the ones outside it); entries may be +-Inf
type Sink struct {
	Min, Max [3]float32
	Outside  bool
}

// syncCount: the library's n_particles has changed: refresh the copy that SetParams sends back and that sizes the buffers
func (e *Engine) syncCount() error {
	return e.ck(C.dsl_get_params(e.h, &e.Params))
}

// SyncCount: after solver steps with an emitter or a sink in place; returns the particle count
func (e *Engine) SyncCount() (int, error) {
	err := e.syncCount()
	return int(e.Params.n_particles), err
}

// AppendParticles: new fluid particles behind the current ones, xyz interleaved; velocities nil: zeros (blocking)
func (e *Engine) AppendParticles(positions, velocities []float32) error {
	if len(positions) == 0 {
		return nil
	}
	var v *C.float
	if len(velocities) > 0 {
		v = (*C.float)(unsafe.Pointer(&velocities[0]))
	}
	if err := e.ck(C.dsl_particles_append(e.h, (*C.float)(unsafe.Pointer(&positions[0])), v, C.size_t(len(positions)/3))); err != nil {
		return err
	}
	return e.syncCount()
}

func (e *Engine) AddEmitter(em Emitter) (id int, err error) {
	var d C.dsl_emitter
	for a := 0; a < 3; a++ {
		d.origin[a], d.u[a], d.v[a], d.velocity[a] = C.float(em.Origin[a]), C.float(em.U[a]), C.float(em.V[a]), C.float(em.Velocity[a])
	}
	d.nu, d.nv, d.period = C.int32_t(em.Nu), C.int32_t(em.Nv), C.int32_t(em.Period)
	if em.Ellipse {
		d.shape = 1
	}
	d.first_step, d.max_layers = C.int64_t(em.FirstStep), C.int64_t(em.MaxLayers)
	var k C.int
	err = e.ck(C.dsl_emitter_add(e.h, &d, &k))
	return int(k), err
}

func (e *Engine) ClearEmitters() error { return e.ck(C.dsl_emitters_clear(e.h)) }

// Emit: one layer of the emitter now, between steps
func (e *Engine) Emit(emitter int) error {
	if err := e.ck(C.dsl_emit(e.h, C.int(emitter))); err != nil {
		return err
	}
	return e.syncCount()
}

func (e *Engine) AddSink(s Sink) (id int, err error) {
	var d C.dsl_sink
	for a := 0; a < 3; a++ {
		d.box_min[a], d.box_max[a] = C.float(s.Min[a]), C.float(s.Max[a])
	}
	if s.Outside {
		d.outside = 1
	}
	var k C.int
	err = e.ck(C.dsl_sink_add(e.h, &d, &k))
	return int(k), err
}

func (e *Engine) ClearSinks() error { return e.ck(C.dsl_sinks_clear(e.h)) }

// RemoveParticles: applies the sinks now; returns how many particles went (blocking)
func (e *Engine) RemoveParticles() (removed int64, err error) {
	var r C.int64_t
	if err = e.ck(C.dsl_particles_remove(e.h, &r)); err != nil {
		return
	}
	return int64(r), e.syncCount()
}

// The frame recorder (include/dslsph.h: dsl_recorder_set): animation frames packed on the device during a run and copied
// to pinned host memory behind the steps that follow -- "Fluid Animation Export" (README.MD:39), in place of the blocking
// read-back of every position after every step (pcisph_gpu_darwin.go:276-279).
const (
	RecVelocity = int(C.DSL_REC_VELOCITY)
	RecDensity  = int(C.DSL_REC_DENSITY)
	RecF32      = int(C.DSL_REC_F32)
	RecQ16      = int(C.DSL_REC_Q16)
	// frames recorded, dropped for want of a released slot, landed and unreleased (all get); milliseconds of the last
	// frame's bounds + pack launches and of its copy (get, blocking; 0 unless TimingEnable(1) held)
	OptRecordFrames  = int(C.DSL_OPT_RECORD_FRAMES)
	OptRecordDropped = int(C.DSL_OPT_RECORD_DROPPED)
	OptRecordReady   = int(C.DSL_OPT_RECORD_READY)
	OptRecordPackMs  = int(C.DSL_OPT_RECORD_PACK_MS)
	OptRecordCopyMs  = int(C.DSL_OPT_RECORD_COPY_MS)
)

// Recorder: a frame at steps s >= FirstStep with (s - FirstStep) % Every == 0, MaxFrames of them (0: no limit); every
// Stride-th particle in host order; Fields = RecVelocity | RecDensity beside the positions; Encoding RecF32 or RecQ16, the
// latter against [BoxMin, BoxMax] or, with AutoBox, each frame's own bounds; Slots frames (1..64) of pinned host memory
type Recorder struct {
	Every, Stride, Fields, Encoding, Slots int
	AutoBox                                bool
	BoxMin, BoxMax                         [3]float32
	FirstStep, MaxFrames                   int64
}

func (r *Recorder) spec() C.dsl_recorder {
	var d C.dsl_recorder
	d.every, d.stride, d.fields = C.int32_t(r.Every), C.int32_t(r.Stride), C.int32_t(r.Fields)
	d.encoding, d.slots = C.int32_t(r.Encoding), C.int32_t(r.Slots)
	if r.AutoBox {
		d.auto_box = 1
	}
	for a := 0; a < 3; a++ {
		d.box_min[a], d.box_max[a] = C.float(r.BoxMin[a]), C.float(r.BoxMax[a])
	}
	d.first_step, d.max_frames = C.int64_t(r.FirstStep), C.int64_t(r.MaxFrames)
	return d
}

// FrameBytes: the size of a frame of n particles under the spec; 0 for a spec SetRecorder would refuse
func (r *Recorder) FrameBytes(n int) int {
	d := r.spec()
	return int(C.dsl_record_frame_bytes(&d, C.int(n)))
}

// SetRecorder: stores the spec and allocates (blocking); nil: the recorder is off and everything is freed
func (e *Engine) SetRecorder(r *Recorder) error {
	if r == nil {
		return e.ck(C.dsl_recorder_set(e.h, nil))
	}
	d := r.spec()
	return e.ck(C.dsl_recorder_set(e.h, &d))
}

// RecordNow: one frame of the current state, between steps
func (e *Engine) RecordNow() error { return e.ck(C.dsl_record_now(e.h)) }

// PollFrames: frames recorded so far, landed and unreleased, dropped; never blocks
func (e *Engine) PollFrames() (recorded, ready, dropped int64, err error) {
	var a, b, c C.int64_t
	err = e.ck(C.dsl_record_poll(e.h, &a, &b, &c))
	return int64(a), int64(b), int64(c), err
}

// NextFrame: the oldest unreleased frame, copied out of its pinned slot and released (waits for its copy only)
func (e *Engine) NextFrame() ([]byte, error) {
	var p unsafe.Pointer
	var n C.size_t
	if err := e.ck(C.dsl_record_peek(e.h, &p, &n)); err != nil {
		return nil, err
	}
	out := C.GoBytes(p, C.int(n))
	return out, e.ck(C.dsl_record_release(e.h))
}

// ReadFrameInto: the oldest unreleased frame copied into buf (at least FrameBytes long) and released, without an allocation
func (e *Engine) ReadFrameInto(buf []byte) error {
	if len(buf) == 0 {
		return errors.New("ReadFrameInto: empty buffer")
	}
	return e.ck(C.dsl_record_read(e.h, unsafe.Pointer(&buf[0]), C.size_t(len(buf))))
}

// AnimationFileHeader: the 16 bytes an animation file starts with: "DSLANIM\0", version 1, zero; the frames follow as
// the library wrote them, each finding the next through its frame_bytes
func AnimationFileHeader() []byte {
	return []byte{'D', 'S', 'L', 'A', 'N', 'I', 'M', 0, 1, 0, 0, 0, 0, 0, 0, 0}
}

// WriteTo: every frame that has been recorded and not released, oldest first, written to w as it is and released; the
// bytes written.  A file is AnimationFileHeader() and then any number of these calls
func (e *Engine) WriteTo(w io.Writer) (int64, error) {
	var total int64
	for {
		recorded, _, _, err := e.PollFrames()
		if err != nil {
			return total, err
		}
		var p unsafe.Pointer
		var n C.size_t
		if recorded == 0 || C.dsl_record_peek(e.h, &p, &n) != C.DSL_OK {
			return total, nil // (nothing unreleased is left)
		}
		k, err := w.Write(C.GoBytes(p, C.int(n)))
		total += int64(k)
		if err != nil {
			return total, err
		}
		if err := e.ck(C.dsl_record_release(e.h)); err != nil {
			return total, err
		}
	}
}
