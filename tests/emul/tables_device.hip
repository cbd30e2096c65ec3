// tables_device.hip -- TEST-ONLY entries over the engine's own table builders (tests/test_tables_build_device.py).
//
// radiative3d_amd/csrc/r3d_tables_build.hip builds, in HBM, everything a run reads that is computed once: the take-off
// set, the Sato-Fehler weights and their cumulative tables, the source patterns, the direction vectors, the polarisation
// pairs and the search guides.  Its builders have external linkage (r3d_tables_build.h) and take any device array of
// (theta, phi) pairs of any length; the engine only ever hands them the icosahedron leaves and its configurations'
// parameters.  Each entry here uploads its input, calls ONE builder, synchronises and copies the result back.
//
// Linked (make devtest) with build/obj/main_tables.o into libr3d_tables_device.so and with build/obj/repro_tables.o into
// libr3d_tables_device_repro.so: the very objects that go into libr3d_hip.so and libr3d_hip_repro.so, not sibling
// compilations.  It stands outside radiative3d_amd/csrc/, is not part of the C-ABI and is loaded by nothing but the tests.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "../../radiative3d_amd/csrc/r3d_pack.h"
#include "../../radiative3d_amd/csrc/r3d_tables_build.h"

using namespace r3d;

namespace {
thread_local char g_error[256] = "";
int fail(const char* what, hipError_t e = hipSuccess) {
  if (e != hipSuccess) std::snprintf(g_error, sizeof g_error, "%s: %s", what, hipGetErrorString(e));
  else std::snprintf(g_error, sizeof g_error, "%s", what);
  return 1;
}
struct DevMem {   // device memory freed when the call returns, whichever way; never of zero bytes
  void* p = nullptr;
  ~DevMem() {
    if (p) (void)hipFree(p);
  }
  hipError_t upload(const void* src, size_t bytes) {
    hipError_t e = hipMalloc(&p, bytes ? bytes : sizeof(double));
    if (e == hipSuccess) e = (src && bytes) ? hipMemcpy(p, src, bytes, hipMemcpyHostToDevice) : hipMemset(p, 0, bytes ? bytes : sizeof(double));
    return e;
  }
  double* d() const { return static_cast<double*>(p); }
};
#define DEVTEST_OK(call)                                   \
  do {                                                     \
    const hipError_t e_ = (call);                          \
    if (e_ != hipSuccess) return fail(#call, e_);          \
  } while (0)
constexpr uint64_t kMaxEntries = 1ull << 24;   // (tables of 128 MB at the most; the tests' longest has 69 633)
constexpr uint32_t kMaxGuideBits = 24;
hipError_t download(void* dst, const DevMem& src, size_t bytes) {
  return bytes ? hipMemcpy(dst, src.p, bytes, hipMemcpyDeviceToHost) : hipSuccess;
}
}  // namespace

extern "C" const char* r3d_devtest_last_error() { return g_error; }

// toa[2 n]: the take-off set of `degree` by build_toa_on_device, which refuses a degree outside 0..12 and n != 20 * 4^degree.
extern "C" int r3d_devtest_toa(int device, int degree, uint64_t n, double* toa) {
  if (!toa) return fail("r3d_devtest_toa: null table");
  if (n > kMaxEntries) return fail("r3d_devtest_toa: too many directions");
  DEVTEST_OK(hipSetDevice(device));
  DevMem dtoa;
  DEVTEST_OK(dtoa.upload(nullptr, 2 * n * sizeof(double)));
  DEVTEST_OK(build_toa_on_device(degree, n, dtoa.d(), nullptr));
  DEVTEST_OK(hipDeviceSynchronize());
  DEVTEST_OK(download(toa, dtoa, 2 * n * sizeof(double)));
  return 0;
}

// xyz[4 n] = {cos theta, cos phi, sin phi, sin theta} of the n (theta, phi) pairs, theta clamped to [min_theta, max_theta].
// (build_toa_xyz_on_device, build_spol_cs_on_device and build_guide_on_device take n >= 1 on trust, as the engine
// guarantees it; n = 0 is refused here, before anything is launched.)
extern "C" int r3d_devtest_toa_xyz(int device, const double* toa, uint64_t n, double min_theta, double max_theta, double* xyz) {
  if (!toa || !xyz) return fail("r3d_devtest_toa_xyz: null table");
  if (n == 0 || n > kMaxEntries) return fail("r3d_devtest_toa_xyz: no directions, or too many");
  DEVTEST_OK(hipSetDevice(device));
  DevMem dtoa, dxyz;
  DEVTEST_OK(dtoa.upload(toa, 2 * n * sizeof(double)));
  DEVTEST_OK(dxyz.upload(nullptr, 4 * n * sizeof(double)));
  DEVTEST_OK(build_toa_xyz_on_device(dtoa.d(), n, min_theta, max_theta, dxyz.d(), nullptr));
  DEVTEST_OK(hipDeviceSynchronize());
  DEVTEST_OK(download(xyz, dxyz, 4 * n * sizeof(double)));
  return 0;
}

// cdf[4 n] (GPP, GPS, GSP, GSS, one after the other), spol[n], totals[4], cos_sums[4] by build_scatterer_tables, which
// refuses n = 0.  het = nu, eps, a, kappa, el, gam0.
extern "C" int r3d_devtest_scatterer(int device, const double het[6], double psdf_numer, const double* toa, uint64_t n, double* cdf,
                                     double* spol, double totals[4], double cos_sums[4]) {
  if (!het || !toa || !cdf || !spol || !totals || !cos_sums) return fail("r3d_devtest_scatterer: null table");
  if (n > kMaxEntries) return fail("r3d_devtest_scatterer: too many directions");
  DEVTEST_OK(hipSetDevice(device));
  DevMem dtoa, dcdf[4], dspol;
  DEVTEST_OK(dtoa.upload(toa, 2 * n * sizeof(double)));
  double* d_cdf[4];
  for (int c = 0; c < 4; c++) {
    DEVTEST_OK(dcdf[c].upload(nullptr, n * sizeof(double)));
    d_cdf[c] = dcdf[c].d();
  }
  DEVTEST_OK(dspol.upload(nullptr, n * sizeof(double)));
  DEVTEST_OK(build_scatterer_tables(het, psdf_numer, dtoa.d(), n, d_cdf, dspol.d(), totals, cos_sums, nullptr));
  DEVTEST_OK(hipDeviceSynchronize());
  for (int c = 0; c < 4; c++) DEVTEST_OK(download(cdf + c * n, dcdf[c], n * sizeof(double)));
  DEVTEST_OK(download(spol, dspol, n * sizeof(double)));
  return 0;
}

// cdf[3 n] (P, SH, SV) and totals[3] by build_source_tables, which refuses n = 0.  moment = xx, yy, zz, xy, xz, yz.
extern "C" int r3d_devtest_source(int device, const double moment[6], const double* toa, uint64_t n, double* cdf, double totals[3]) {
  if (!moment || !toa || !cdf || !totals) return fail("r3d_devtest_source: null table");
  if (n > kMaxEntries) return fail("r3d_devtest_source: too many directions");
  DEVTEST_OK(hipSetDevice(device));
  DevMem dtoa, dcdf[3];
  DEVTEST_OK(dtoa.upload(toa, 2 * n * sizeof(double)));
  double* d_cdf[3];
  for (int c = 0; c < 3; c++) {
    DEVTEST_OK(dcdf[c].upload(nullptr, n * sizeof(double)));
    d_cdf[c] = dcdf[c].d();
  }
  DEVTEST_OK(build_source_tables(moment, dtoa.d(), n, d_cdf, totals, nullptr));
  DEVTEST_OK(hipDeviceSynchronize());
  for (int c = 0; c < 3; c++) DEVTEST_OK(download(cdf + c * n, dcdf[c], n * sizeof(double)));
  return 0;
}

// cs[2 n]: (cosine, sine) of the n angles spol.
extern "C" int r3d_devtest_spol_cs(int device, const double* spol, uint64_t n, double* cs) {
  if (!spol || !cs) return fail("r3d_devtest_spol_cs: null table");
  if (n == 0 || n > kMaxEntries) return fail("r3d_devtest_spol_cs: no angles, or too many");
  DEVTEST_OK(hipSetDevice(device));
  DevMem dspol, dcs;
  DEVTEST_OK(dspol.upload(spol, n * sizeof(double)));
  DEVTEST_OK(dcs.upload(nullptr, 2 * n * sizeof(double)));
  DEVTEST_OK(build_spol_cs_on_device(dspol.d(), n, dcs.d(), nullptr));
  DEVTEST_OK(hipDeviceSynchronize());
  DEVTEST_OK(download(cs, dcs, 2 * n * sizeof(double)));
  return 0;
}

// cells[2^bits] (raw 64-byte GuideCell records) of the cumulative table cdf[n], by build_guide_on_device ...
extern "C" int r3d_devtest_guide(int device, const double* cdf, uint64_t n, uint32_t bits, void* cells) {
  if (!cdf || !cells) return fail("r3d_devtest_guide: null table");
  if (n == 0 || n > kMaxEntries || bits > kMaxGuideBits) return fail("r3d_devtest_guide: table or guide out of range");
  DEVTEST_OK(hipSetDevice(device));
  const size_t bytes = (size_t(1) << bits) * sizeof(GuideCell);
  DevMem dcdf, dguide;
  DEVTEST_OK(dcdf.upload(cdf, n * sizeof(double)));
  DEVTEST_OK(dguide.upload(nullptr, bytes));
  DEVTEST_OK(build_guide_on_device(dcdf.d(), n, bits, static_cast<GuideCell*>(dguide.p), nullptr));
  DEVTEST_OK(hipDeviceSynchronize());
  DEVTEST_OK(download(cells, dguide, bytes));
  return 0;
}

// ... and by build_guide_cells (r3d_pack.h) on the host: the same layout, no GPU.
extern "C" int r3d_devtest_host_guide(const double* cdf, uint64_t n, uint32_t bits, void* cells) {
  if (!cdf || !cells) return fail("r3d_devtest_host_guide: null table");
  if (n == 0 || n > kMaxEntries || bits > kMaxGuideBits) return fail("r3d_devtest_host_guide: table or guide out of range");
  std::vector<GuideCell> g;
  build_guide_cells(cdf, n, bits, g);
  std::memcpy(cells, g.data(), g.size() * sizeof(GuideCell));
  return 0;
}

// The width the engine chooses for the guides of tables of n entries (r3d_pack.h guide_bits_for).
extern "C" uint32_t r3d_devtest_guide_bits_for(uint64_t n) { return guide_bits_for(n); }
