// physics_device.hip -- TEST-ONLY device build of the per-lane physics, case by case (tests/test_physics_device.py).
//
// The evaluators of tests/emul/physics_cases.h -- the functions the host loop of tests/emul/emul.cpp runs row by row --
// compiled by hipcc for gfx950 and run one lane per case, and the two pieces of r3d_physics.h that exist in a device
// build only: the tetra boundary search by four lanes per history (tet_fast_exit_quad, the drain kernel's) and the
// address-space-1 path of sample_cdf_guided.  Built twice (make devtest): with the engine's flags, and with the
// reproducible build's (-DR3D_REPRODUCIBLE -ffp-contract=off).
//
// It is a SIBLING compilation of the same text under the same flags, with its own inlining and schedule: not the code
// object of the traversal kernels.  (Only build_guide_on_device, for the guided draws, is the engine's own object:
// build/obj/main_tables.o resp. repro_tables.o is linked in.)  It stands outside radiative3d_amd/csrc/, is not part of the C-ABI and is loaded by
// nothing but the tests.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

// (as in the kernels: the host emulation's tallies are nothing in a device build)
#define R3D_COUNT_SLOW_MOVE() ((void)0)
#define R3D_LOC_REASON(k, mask) ((void)0)
#include "../../radiative3d_amd/csrc/r3d_pack.h"
#include "../../radiative3d_amd/csrc/r3d_physics.h"
#include "../../radiative3d_amd/csrc/r3d_tables_build.h"
#include "physics_cases.h"

using namespace r3d;
using namespace r3d_cases;

namespace {
thread_local char g_error[256] = "";
int fail(const char* what, hipError_t e = hipSuccess) {
  if (e != hipSuccess) std::snprintf(g_error, sizeof g_error, "%s: %s", what, hipGetErrorString(e));
  else std::snprintf(g_error, sizeof g_error, "%s", what);
  return 1;
}
struct DevMem {   // device memory freed when the call returns, whichever way
  void* p = nullptr;
  ~DevMem() {
    if (p) (void)hipFree(p);
  }
  hipError_t upload(const void* src, size_t bytes) {
    hipError_t e = hipMalloc(&p, bytes);
    if (e == hipSuccess && src) e = hipMemcpy(p, src, bytes, hipMemcpyHostToDevice);
    return e;
  }
};
#define DEVTEST_OK(call)                                   \
  do {                                                     \
    const hipError_t e_ = (call);                          \
    if (e_ != hipSuccess) return fail(#call, e_);          \
  } while (0)
constexpr unsigned kBlock = 256;
unsigned blocks_for(uint64_t lanes) { return (unsigned)((lanes + kBlock - 1) / kBlock); }
constexpr uint64_t kMaxCases = 1ull << 26;   // (a grid of 32-bit block counts and tables of a few GB at the most)

// one lane per case; the votes of a partial last wave see its active lanes only
// (a kernel per family and form: each the size of the code it holds, as the traversal kernels' phases are)
template <int FAMILY, bool FLAT>
__global__ void eval_kernel(const double* __restrict__ in, double* __restrict__ out, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  eval_row<FLAT>(FAMILY, in, out, i);
}
template <int FAMILY, bool FLAT>
void launch_eval(const double* in, double* out, uint64_t n) {
  eval_kernel<FAMILY, FLAT><<<dim3(blocks_for(n)), dim3(kBlock)>>>(in, out, n);
}

// lanes 4j .. 4j+3 hold tetra case j; lane f reads face f of the record from memory, as step_move does
__global__ void quad_kernel(const CellTet* __restrict__ cells, const double* __restrict__ in, double* __restrict__ out, uint64_t n) {
  const uint64_t lane = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t j = lane >> 2;
  if (j >= n) return;   // (whole quads leave together)
#if defined(__HIP_DEVICE_COMPILE__)   // (tet_fast_exit_quad exists in the device pass only, as in step_move)
  const unsigned fl = (unsigned)(lane & 3u);
  const CellTet c = cells[j];
  const V3 quad_n = v3(cells[j].n[fl]);
  const double quad_d = cells[j].d[fl];
  const double* r = in + j * TET_IN;
  const Phonon p = search_phonon(r + 33, r + 36);
  TetLocal L;
  const TetFast F = tet_fast_exit_quad(c, quad_n, quad_d, p, L);
  tet_finish_row(c, p, L, F, out + lane * SEARCH_OUT);
#endif
}

__global__ void guided_kernel(const double* __restrict__ cdf, const GuideCell* __restrict__ guide, uint32_t bits, double total,
                              const double* __restrict__ u, uint64_t* __restrict__ out, uint64_t m) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  out[i] = sample_cdf_guided(cdf, guide, bits, total, u[i]);
}
}  // namespace

extern "C" const char* r3d_devtest_last_error() { return g_error; }

// Rows `in` (family's input width) -> rows `out` (its output width), evaluated on `device`.  family: 0 R/T events, 1 bends,
// 2 rotations, 3 tetra search, 4 shell search; flat_form: the flat-face form of families 0 and 1.  0, or 1 with an error text.
extern "C" int r3d_devtest_eval(int device, int family, int flat_form, const double* in, double* out, uint64_t n) {
  if (!in || !out) return fail("r3d_devtest_eval: null table");
  if (family < 0 || family >= FAM_COUNT) return fail("r3d_devtest_eval: unknown family");
  if (n > kMaxCases) return fail("r3d_devtest_eval: too many cases");
  if (n == 0) return 0;
  DEVTEST_OK(hipSetDevice(device));
  const size_t in_bytes = n * in_width(family) * sizeof(double), out_bytes = n * out_width(family) * sizeof(double);
  DevMem din, dout;
  DEVTEST_OK(din.upload(in, in_bytes));
  DEVTEST_OK(dout.upload(nullptr, out_bytes));
  DEVTEST_OK(hipMemset(dout.p, 0, out_bytes));
  const double* i_ = (const double*)din.p;
  double* o_ = (double*)dout.p;
  switch (family) {
    case FAM_RT: flat_form ? launch_eval<FAM_RT, true>(i_, o_, n) : launch_eval<FAM_RT, false>(i_, o_, n); break;
    case FAM_BEND: flat_form ? launch_eval<FAM_BEND, true>(i_, o_, n) : launch_eval<FAM_BEND, false>(i_, o_, n); break;
    case FAM_ROT: launch_eval<FAM_ROT, false>(i_, o_, n); break;
    case FAM_TET: launch_eval<FAM_TET, false>(i_, o_, n); break;
    default: launch_eval<FAM_SHELL, false>(i_, o_, n); break;
  }
  DEVTEST_OK(hipGetLastError());
  DEVTEST_OK(hipDeviceSynchronize());
  DEVTEST_OK(hipMemcpy(out, dout.p, out_bytes, hipMemcpyDeviceToHost));
  return 0;
}

// The tetra search by quads: `in` n tetra rows, `out` 4 n search rows (row 4 j + f: what lane f of quad j holds).
extern "C" int r3d_devtest_quad(int device, const double* in, double* out, uint64_t n) {
  if (!in || !out) return fail("r3d_devtest_quad: null table");
  if (n > kMaxCases / 4) return fail("r3d_devtest_quad: too many cases");
  if (n == 0) return 0;
  std::vector<CellTet> cells(n);
  for (uint64_t j = 0; j < n; j++) tet_cell_of_row(in + j * TET_IN, cells[j]);
  DEVTEST_OK(hipSetDevice(device));
  const size_t out_bytes = 4 * n * SEARCH_OUT * sizeof(double);
  DevMem dcells, din, dout;
  DEVTEST_OK(dcells.upload(cells.data(), n * sizeof(CellTet)));
  DEVTEST_OK(din.upload(in, n * TET_IN * sizeof(double)));
  DEVTEST_OK(dout.upload(nullptr, out_bytes));
  DEVTEST_OK(hipMemset(dout.p, 0, out_bytes));
  quad_kernel<<<dim3(blocks_for(4 * n)), dim3(kBlock)>>>((const CellTet*)dcells.p, (const double*)din.p, (double*)dout.p, n);
  DEVTEST_OK(hipGetLastError());
  DEVTEST_OK(hipDeviceSynchronize());
  DEVTEST_OK(hipMemcpy(out, dout.p, out_bytes, hipMemcpyDeviceToHost));
  return 0;
}

// out[i] = sample_cdf_guided(cdf, guide, bits, cdf[n - 1], u[i]) on the device (bits = 0: the width the engine chooses for a
// table of n entries).  The guide is built here by build_guide_cells, or, with guide_on_device, in HBM by the engine's own
// build_guide_on_device (the library is linked with the engine's table object): the builder of every guide a run reads.
extern "C" int r3d_devtest_guided(int device, const double* cdf, uint64_t n, uint32_t bits, const double* u, uint64_t m,
                                  uint64_t* out, int guide_on_device) {
  if (!cdf || !u || !out) return fail("r3d_devtest_guided: null table");
  if (n == 0 || n > (1ull << 31) || bits > 24 || m > kMaxCases) return fail("r3d_devtest_guided: table or guide out of range");
  if (m == 0) return 0;
  for (uint64_t i = 0; i < m; i++)
    if (!(u[i] >= 0.0 && u[i] <= 1.0)) return fail("r3d_devtest_guided: a draw outside [0, 1]");
  if (!bits) bits = guide_bits_for(n);
  std::vector<GuideCell> cells;
  if (!guide_on_device) build_guide_cells(cdf, n, bits, cells);
  DEVTEST_OK(hipSetDevice(device));
  DevMem dcdf, dguide, du, dout;
  DEVTEST_OK(dcdf.upload(cdf, n * sizeof(double)));
  DEVTEST_OK(dguide.upload(guide_on_device ? nullptr : cells.data(), (size_t(1) << bits) * sizeof(GuideCell)));
  if (guide_on_device) {
    DEVTEST_OK(hipMemset(dguide.p, 0, (size_t(1) << bits) * sizeof(GuideCell)));
    DEVTEST_OK(build_guide_on_device((const double*)dcdf.p, n, bits, (GuideCell*)dguide.p, nullptr));
    DEVTEST_OK(hipDeviceSynchronize());
  }
  DEVTEST_OK(du.upload(u, m * sizeof(double)));
  DEVTEST_OK(dout.upload(nullptr, m * sizeof(uint64_t)));
  DEVTEST_OK(hipMemset(dout.p, 0, m * sizeof(uint64_t)));
  guided_kernel<<<dim3(blocks_for(m)), dim3(kBlock)>>>((const double*)dcdf.p, (const GuideCell*)dguide.p, bits, cdf[n - 1],
                                                       (const double*)du.p, (uint64_t*)dout.p, m);
  DEVTEST_OK(hipGetLastError());
  DEVTEST_OK(hipDeviceSynchronize());
  DEVTEST_OK(hipMemcpy(out, dout.p, m * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return 0;
}
