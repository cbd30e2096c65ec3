// cmdline.cpp -- see cmdline.hpp.
#include "cmdline.hpp"

#include <cctype>
#include <cmath>
#include <cstdlib>
#include <deque>
#include <iostream>
#include <map>

#include "batch_products.hpp"
#include "dataout.hpp"

namespace {

enum OptID {
  OPT_FREQ, OPT_NUMBER, OPT_TTLIVE, OPT_TOA, OPT_COMPSELECT, OPT_MODARGS, OPT_CYLRANGE,
  OPT_FLATTEN, OPT_EARTHRAD, OPT_EVENT_MT, OPT_EVENT_LOC, OPT_OVR_MFP, OPT_NODEFLECT,
  OPT_REPORTS, OPT_REPORT_FILE, OPT_OUTDIR, OPT_OCSRAW, OPT_SEISBINS, OPT_SEISBINSIZE,
  OPT_SEISARRAY, OPT_SEIS_P2P, OPT_SEIS_P2PW, OPTM_HELP, OPTM_DUMPGRID, OPTM_PARAMOUTFN,
  OPTM_RTTEST, OPTM_EVENTTEST, OPTM_RUNSIM, OPTX_SEED, OPTX_GPUS, OPTX_DEVTABLES, OPTX_HOSTTABLES,
  OPTX_DEVICES, OPTX_SCATGRID, OPTX_SCATGRID_FILE, OPTX_ERRBATCHES,
  OPTX_SCATVIEWS, OPTX_SCATVIEW_AZI, OPTX_NO_SCATGRID_FILE, OPTX_SCATMAPS, OPTX_JOBERRBATCHES,
  OPTX_LAPSE, OPTX_LAPSE_AXES, OPTX_LAPSE_GEOSPREAD, OPTX_LAPSE_RANGES, OPTX_LAPSE_ARRAY,
  OPTX_TTIMAGE, OPTX_TTIMAGE_ARRAY, OPTX_TTIMAGE_AXES, OPTX_TTIMAGE_FIT, OPTX_TTIMAGE_NORMCURVE,
  OPTX_TARGET, OPTX_TARGET_ARRAY, OPTX_TARGET_COMPONENTS,
  OPTX_ENVSHAPE, OPTX_ENVSHAPE_ARRAY, OPTX_ENVSHAPE_AXES,
  OPTX_ENVFIT, OPTX_ENVFIT_ARRAY, OPTX_ENVFIT_AXES, OPTX_ENVFIT_ENERGY,
  OPTX_SLANT, OPTX_SLANT_ARRAY, OPTX_SLANT_AXES, OPTX_SLANT_ENERGY, OPTX_SLANT_RANGEPOWER, OPTX_SLANT_WINDOWS,
  OPTX_CONTRAST, OPTX_CONTRAST_ARGS, OPTX_CONTRAST_ARRAY, OPTX_CONTRAST_AXES, OPTX_CONTRAST_WINDOWS, OPTX_CONTRAST_REGIONS,
  OPTX_CONTRAST_RANGEPOWER, OPTX_CONTRAST_SEED, OPTX_CONTRAST_NUMBER,
  OPTX_BANDS, OPTX_BANDS_ARRAY, OPTX_BANDS_AXES, OPTX_BANDS_SEED
};

const std::map<std::string, OptID>& option_table() {
  static const std::map<std::string, OptID> t = {
      {"-F", OPT_FREQ}, {"--frequency", OPT_FREQ},
      {"-N", OPT_NUMBER}, {"--num-phonons", OPT_NUMBER},
      {"-T", OPT_TTLIVE}, {"--timetolive", OPT_TTLIVE},
      {"-A", OPT_TOA}, {"--toa-degree", OPT_TOA},
      {"--grid-compiled", OPT_COMPSELECT},
      {"--model-args", OPT_MODARGS}, {"--model-compiled-args", OPT_MODARGS},
      {"--range", OPT_CYLRANGE}, {"--cylinder-range", OPT_CYLRANGE},
      {"--flatten", OPT_FLATTEN},
      {"--earthrad", OPT_EARTHRAD}, {"--earthradius", OPT_EARTHRAD},
      {"-E", OPT_EVENT_MT}, {"--source", OPT_EVENT_MT},
      {"-L", OPT_EVENT_LOC}, {"--source-loc", OPT_EVENT_LOC},
      {"--mfpoverride", OPT_OVR_MFP}, {"--overridemfp", OPT_OVR_MFP},
      {"--nodeflect", OPT_NODEFLECT}, {"--no-deflect", OPT_NODEFLECT},
      {"--reports", OPT_REPORTS}, {"--report-file", OPT_REPORT_FILE},
      {"--output-dir", OPT_OUTDIR},
      {"--ocsnotransform", OPT_OCSRAW}, {"--ocsraw", OPT_OCSRAW},
      {"--binspercycle", OPT_SEISBINS}, {"--bins", OPT_SEISBINS},
      {"--binsize", OPT_SEISBINSIZE},
      {"--seis-array", OPT_SEISARRAY},
      {"--seis-p2p", OPT_SEIS_P2P}, {"--seis-p2pw", OPT_SEIS_P2PW},
      {"--help", OPTM_HELP}, {"--dump-grid", OPTM_DUMPGRID},
      {"--mparams-outfile", OPTM_PARAMOUTFN},
      {"--rtcoef-test", OPTM_RTTEST}, {"--event-test", OPTM_EVENTTEST},
      {"--run-simulation", OPTM_RUNSIM}, {"--run-sim", OPTM_RUNSIM},
      {"--seed", OPTX_SEED}, {"--gpus", OPTX_GPUS}, {"--device-tables", OPTX_DEVTABLES},
      {"--host-tables", OPTX_HOSTTABLES}, {"--devices", OPTX_DEVICES},
      {"--scatter-grid", OPTX_SCATGRID}, {"--scatter-grid-file", OPTX_SCATGRID_FILE},
      {"--error-batches", OPTX_ERRBATCHES}, {"--job-error-batches", OPTX_JOBERRBATCHES},
      {"--scatter-views", OPTX_SCATVIEWS}, {"--scatter-view-azimuth", OPTX_SCATVIEW_AZI},
      {"--no-scatter-grid-file", OPTX_NO_SCATGRID_FILE}, {"--scatter-maps", OPTX_SCATMAPS},
      {"--lapse-windows", OPTX_LAPSE}, {"--lapse-axes", OPTX_LAPSE_AXES}, {"--lapse-geospread", OPTX_LAPSE_GEOSPREAD},
      {"--lapse-ranges", OPTX_LAPSE_RANGES}, {"--lapse-array", OPTX_LAPSE_ARRAY},
      {"--ttimage", OPTX_TTIMAGE}, {"--ttimage-array", OPTX_TTIMAGE_ARRAY}, {"--ttimage-axes", OPTX_TTIMAGE_AXES},
      {"--ttimage-fit", OPTX_TTIMAGE_FIT}, {"--ttimage-normcurve", OPTX_TTIMAGE_NORMCURVE},
      {"--target-error", OPTX_TARGET}, {"--target-array", OPTX_TARGET_ARRAY}, {"--target-components", OPTX_TARGET_COMPONENTS},
      {"--envelope-shape", OPTX_ENVSHAPE}, {"--envelope-array", OPTX_ENVSHAPE_ARRAY}, {"--envelope-axes", OPTX_ENVSHAPE_AXES},
      {"--envelope-fit", OPTX_ENVFIT}, {"--envelope-fit-array", OPTX_ENVFIT_ARRAY}, {"--envelope-fit-axes", OPTX_ENVFIT_AXES},
      {"--envelope-fit-energy", OPTX_ENVFIT_ENERGY},
      {"--slant-stack", OPTX_SLANT}, {"--slant-array", OPTX_SLANT_ARRAY}, {"--slant-axes", OPTX_SLANT_AXES},
      {"--slant-energy", OPTX_SLANT_ENERGY}, {"--slant-range-power", OPTX_SLANT_RANGEPOWER}, {"--slant-windows", OPTX_SLANT_WINDOWS},
      {"--array-contrast", OPTX_CONTRAST}, {"--contrast-model-args", OPTX_CONTRAST_ARGS}, {"--contrast-array", OPTX_CONTRAST_ARRAY},
      {"--contrast-axes", OPTX_CONTRAST_AXES}, {"--contrast-windows", OPTX_CONTRAST_WINDOWS},
      {"--contrast-regions", OPTX_CONTRAST_REGIONS}, {"--contrast-range-power", OPTX_CONTRAST_RANGEPOWER},
      {"--contrast-seed", OPTX_CONTRAST_SEED}, {"--contrast-num-phonons", OPTX_CONTRAST_NUMBER},
      {"--envelope-bands", OPTX_BANDS}, {"--bands-array", OPTX_BANDS_ARRAY}, {"--bands-axes", OPTX_BANDS_AXES},
      {"--bands-seed", OPTX_BANDS_SEED}};
  return t;
}

bool looks_like_option(const std::string& s) {
  return s.size() >= 2 && s[0] == '-' && (s[1] == '-' || std::isalpha((unsigned char)s[1]));
}

// One option with its comma-separated value list.
struct Opt {
  std::string token;
  std::deque<std::string> values;

  bool has() const { return !values.empty(); }
  std::string text() {
    if (values.empty()) throw Runtime("Required value not provided for " + token + ".");
    std::string v = values.front();
    values.pop_front();
    return v;
  }
  Real real() {
    std::string v = text();
    char* end = nullptr;
    Real r = std::strtod(v.c_str(), &end);
    if (end == v.c_str() || *end != '\0')
      throw Runtime("Invalid value: cannot interpret '" + v + "' as type Real.");
    return r;
  }
  long integer() {
    std::string v = text();
    if (!v.empty()) {
      const char* zeros = nullptr;
      switch (v.back()) {
        case 'K': zeros = "000"; break;
        case 'M': zeros = "000000"; break;
        case 'B': zeros = "000000000"; break;
      }
      if (zeros) v = v.substr(0, v.size() - 1) + zeros;
    }
    char* end = nullptr;
    long r = std::strtol(v.c_str(), &end, 10);
    if (end == v.c_str() || *end != '\0')
      throw Runtime("Invalid value: cannot interpret '" + v + "' as type Integer.");
    return r;
  }
  R3::XYZ xyz() {
    Real x = real(), y = real(), z = real();
    return {x, y, z};
  }
};

// Linear receiver array between two points given as raw coordinate triples
// (reference main.cpp:340-392): positions AND gather radii are interpolated in
// the user's coordinate tuple space, not along geodesics.
void add_p2p_array(Opt& o, ModelParams& par, bool force_wavelengths) {
  const bool two_gathers = (o.values.size() == 10);
  R3::XYZ origin = o.xyz(), dest = o.xyz();
  Real offset = o.real();
  Real g1 = o.real(), g2 = g1;
  if (two_gathers) g2 = o.real();
  long n = o.integer();
  const R3::XYZ span = origin.VectorTo(dest);
  const R3::XYZ dir = span.Unit();
  const R3::XYZ begin = origin + dir.ScaledBy(offset);
  const Real gap = n > 1 ? begin.VectorTo(dest).Mag() / (n - 1) : 0.0;
  static bool warned = false;
  for (long i = 0; i < n; i++) {
    R3::XYZ p = begin + dir.ScaledBy(i * gap);
    Real frac = origin.VectorTo(p).Mag() / span.Mag();
    Real gather = g1 + frac * (g2 - g1);
    if (!warned || force_wavelengths) {
      std::cout << "Warning: Seis array interpolation ignores coordinate "
                << "system and could produce distorted results.\n";
      warned = true;
    }
    EarthCoords::Generic at(p.x(), p.y(), p.z());
    if (two_gathers && !force_wavelengths)
      par.AddSeismometerFixedRadius(at, ModelParams::AX_RTZ, gather);
    else
      par.AddSeismometerByWavelength(at, ModelParams::AX_RTZ, gather);
  }
}

void set_source(Opt& o, ModelParams& par) {
  std::string kind = o.text();
  if (kind == "EQ") {
    par.EventSourceMT = Tensor::USGS(0, -1, 1, 0, 0, 0);
  } else if (kind == "EXPL") {
    par.EventSourceMT = Tensor::USGS(1, 1, 1, 0, 0, 0);
  } else if (kind == "USGS") {
    if (o.values.size() < 6)
      throw Runtime("USGS keyword expects six numeric moment tensor elements.");
    Real m[6];
    for (Real& v : m) v = o.real();
    par.EventSourceMT = Tensor::USGS(m[0], m[1], m[2], m[3], m[4], m[5]);
  } else if (kind == "SDR") {
    std::vector<Real> a;
    while (o.has()) a.push_back(o.real());
    auto iso_of = [](Real iso) {
      return (iso > 1.0 || iso < -1.0) ? Tensor::SDR::IsoFracFromIsoAngle(iso) : iso;
    };
    if (a.size() == 3) {
      par.EventSourceMT = Tensor::SDR(a[0], a[1], a[2]);
    } else if (a.size() == 4) {
      par.EventSourceMT = Tensor::SDR(a[0], a[1], a[2], iso_of(a[3]));
    } else if (a.size() == 5) {
      Real iso = a[3], moment = a[4];
      if (moment == 0.0) {  // old argument order (moment, iso)
        std::swap(iso, moment);
        std::cout << "Warning: SDR Event Specification: Swapped iso and moment arguments.\n"
                  << "Warning: (Note new argument order: "
                  << "--source=SDR,strike,dip,rake,iso,moment)\n";
      }
      par.EventSourceMT = Tensor::SDR(a[0], a[1], a[2], iso_of(iso), moment);
    } else {
      throw Runtime("SDR keyword expects SDR,strike,dip,rake[,iso[,moment]].");
    }
  } else {
    throw Runtime(kind + " is not a valid source mechanism keyword.");
  }
}

// The shards that --gpus / --devices name.
unsigned long shard_count(const MissionParams& mission) {
  return mission.Devices.empty() ? (unsigned long)std::max(1, mission.Gpus) : mission.Devices.size();
}

}  // namespace

void ParseCommandLine(const std::vector<std::string>& tokens, ModelParams& par,
                      MissionParams& mission) {
  for (size_t i = 0; i < tokens.size(); i++) {
    const std::string& tk = tokens[i];
    if (!looks_like_option(tk)) continue;  // stray value: a no-op, as in the reference
    Opt o;
    std::string vals;
    size_t eq = tk.find('=');
    if (tk[1] == '-' && eq != std::string::npos) {
      o.token = tk.substr(0, eq);
      vals = tk.substr(eq + 1);
    } else {
      o.token = tk;
      if (i + 1 < tokens.size() && !looks_like_option(tokens[i + 1])) vals = tokens[++i];
    }
    for (size_t p = 0; !vals.empty();) {
      size_t c = vals.find(',', p);
      o.values.push_back(vals.substr(p, c == std::string::npos ? c : c - p));
      if (c == std::string::npos) break;
      p = c + 1;
    }
    auto it = option_table().find(o.token);
    if (it == option_table().end()) throw Runtime("Unrecognized option: " + o.token);

    switch (it->second) {
      case OPT_FREQ: par.Frequency = o.real(); break;
      case OPT_NUMBER: par.NumPhonons = o.integer(); break;
      case OPT_TTLIVE: par.PhononTTL = o.real(); break;
      case OPT_TOA: par.TOA_Degree = (int)o.integer(); break;
      case OPT_COMPSELECT:
        par.GridSource = ModelParams::GRID_COMPILED;
        par.CompiledSelector = o.has() ? (int)o.integer() : 0;
        break;
      case OPT_MODARGS:
        while (o.has()) par.CompiledArgs.push_back(o.real());
        break;
      case OPT_CYLRANGE: par.CylinderRange = o.real(); break;
      case OPT_FLATTEN: par.Flatten = true; break;
      case OPT_EARTHRAD: par.EarthRadius = o.real(); break;
      case OPT_EVENT_MT: set_source(o, par); break;
      case OPT_EVENT_LOC: {
        Real x = o.real(), y = o.real(), z = o.real();
        par.EventSourceLoc = EarthCoords::Generic(x, y, z);
      } break;
      case OPT_OVR_MFP:
        par.OverrideMFP = true;
        par.MFPOverride[0] = o.real();
        par.MFPOverride[1] = o.real();
        break;
      case OPT_NODEFLECT: par.NoDeflect = true; break;
      case OPT_REPORTS:
        mission.Reports.clear();
        if (!o.has()) mission.Reports = "ALL_ON";
        while (o.has()) {
          std::string kw = o.text();
          ApplyReportKeyword(0, kw);   // (throws for a word that is no keyword)
          mission.Reports += (mission.Reports.empty() ? "" : ",") + kw;
        }
        break;
      case OPT_REPORT_FILE: mission.ReportFile = o.text(); break;
      case OPT_OUTDIR: mission.OutputDir = o.text(); break;
      case OPT_OCSRAW: par.OcsRaw = true; break;
      case OPT_SEISBINS:
        par.TimeBinsPerCycle = o.real();
        par.TimeBinSize = 0;
        break;
      case OPT_SEISBINSIZE:
        par.TimeBinsPerCycle = 0;
        par.TimeBinSize = o.real();
        break;
      case OPT_SEISARRAY:
        throw Runtime("Arg: --seisarray: Disabled; use --seis-p2p instead.");
      case OPT_SEIS_P2P: add_p2p_array(o, par, false); break;
      case OPT_SEIS_P2PW: add_p2p_array(o, par, true); break;
      case OPTM_HELP: mission.bHelpMsg = true; break;
      case OPTM_RUNSIM: mission.bRunSim = true; break;
      case OPTM_DUMPGRID: mission.bDumpGrid = true; break;
      case OPTM_PARAMOUTFN:
        mission.bOutputModParamsOctv = true;
        mission.FNModParamsOctv = o.text();
        break;
      case OPTM_RTTEST: mission.bRTCoefTest = true, mission.bRunSim = false; break;
      case OPTM_EVENTTEST: mission.bSourcePatternTest = true, mission.bRunSim = false; break;
      case OPTX_SEED: mission.Seed = (unsigned long)std::strtoull(o.text().c_str(), nullptr, 0); break;
      case OPTX_GPUS: mission.Gpus = (int)o.integer(); break;
      case OPTX_DEVICES:
        mission.Devices.clear();
        while (o.has()) mission.Devices.push_back((int)o.integer());
        if (mission.Devices.empty()) throw Runtime("--devices needs at least one device index.");
        break;
      case OPTX_SCATGRID: {
        long v[4];
        for (int k = 0; k < 4; k++) v[k] = o.integer();
        for (int k = 0; k < 3; k++) mission.GridLo[k] = o.real();
        for (int k = 0; k < 3; k++) mission.GridHi[k] = o.real();
        for (int k = 0; k < 3; k++) {
          if (v[k] < 1 || v[k] > 0xFFFFFFFFL || !(mission.GridHi[k] > mission.GridLo[k]))
            throw Runtime("--scatter-grid=NX,NY,NZ,FRAMES,X0,Y0,Z0,X1,Y1,Z1: cell counts must be positive (and below 2^32) and X1 > X0 etc.");
          mission.GridDims[k] = (unsigned)v[k];
        }
        if (v[3] < 1 || v[3] > 0xFFFFFFFFL) throw Runtime("--scatter-grid: FRAMES must be positive (and below 2^32).");
        mission.GridFrames = (unsigned)v[3];
        mission.bScatterGrid = true;
        break;
      }
      case OPTX_SCATGRID_FILE: mission.ScatterGridFile = o.text(); break;
      case OPTX_ERRBATCHES: {
        const long b = o.integer();
        if (b < 2 || b > 64)
          throw Runtime("--error-batches=B: the number of batches must be 2 .. 64 (got " + std::to_string(b) + ").");
        mission.ErrorBatches = (unsigned)b;
        break;
      }
      case OPTX_JOBERRBATCHES: {
        const long b = o.integer();
        if (b < 2 || b > 0x7FFFFFFFL)
          throw Runtime("--job-error-batches=N: the job needs at least 2 batches (got " + std::to_string(b) + ").");
        mission.JobErrorBatches = (unsigned)b;
        break;
      }
      case OPTX_SCATVIEWS: {
        const long g = o.has() ? o.integer() : 1;
        if (g < 1 || g > 0xFFFFFFFFL)
          throw Runtime("--scatter-views[=GROUP]: GROUP, the grid frames per frame of the views, must be positive (got " +
                        std::to_string(g) + ").");
        mission.bScatterViews = true;
        mission.ViewGroup = (unsigned)g;
        break;
      }
      case OPTX_SCATVIEW_AZI:
        mission.ViewAzimuth = o.real();
        mission.ViewHalfWidth = o.real();
        if (!(mission.ViewHalfWidth >= 0)) throw Runtime("--scatter-view-azimuth=AZI,HALFWIDTH: HALFWIDTH must not be negative.");
        mission.bViewAzimuth = true;
        break;
      case OPTX_NO_SCATGRID_FILE: mission.bNoScatterGridFile = true; break;
      case OPTX_SCATMAPS: {
        const long c = o.has() ? o.integer() : 1;
        if (c < 1 || c > 0xFFFFFFFFL)
          throw Runtime("--scatter-maps[=MINCOUNT]: MINCOUNT, the events a cell needs in a frame to count as reached, must be "
                        "positive (got " + std::to_string(c) + ").");
        mission.bScatterMaps = true;
        mission.MapMinCount = (unsigned)c;
        break;
      }
      case OPTX_LAPSE: {
        if (o.has()) {
          for (int k = 0; k < 2; k++) mission.LapseEdge[k] = o.real();
          for (int k = 0; k < 4; k++) mission.LapseWindows[k] = o.real();
        }
        const double* w = mission.LapseWindows;
        if (!(mission.LapseEdge[0] > 0) || !std::isfinite(mission.LapseEdge[0]) || !std::isfinite(mission.LapseEdge[1]) ||
            !(w[1] >= w[0]) || !(w[3] >= w[2]) || !std::isfinite(w[0] + w[1] + w[2] + w[3]))
          throw Runtime("--lapse-windows[=V,T0,B1,E1,B2,E2]: the phase velocity V must be positive, each window's end not "
                        "before its start, and every number finite.");
        mission.bLapse = true;
        break;
      }
      case OPTX_LAPSE_AXES:
        for (int k = 0; k < 3; k++) mission.LapseAxes[k] = o.real();
        if (!std::isfinite(mission.LapseAxes[0] + mission.LapseAxes[1] + mission.LapseAxes[2]))
          throw Runtime("--lapse-axes=X,Y,Z: the weights must be finite.");
        mission.LapseCompanion = "--lapse-axes";
        break;
      case OPTX_LAPSE_GEOSPREAD:
        mission.LapseGeoSpread = o.real();
        if (!std::isfinite(mission.LapseGeoSpread)) throw Runtime("--lapse-geospread=G: G must be finite.");
        mission.LapseCompanion = "--lapse-geospread";
        break;
      case OPTX_LAPSE_RANGES:
        for (int k = 0; k < 3; k++) mission.LapseRanges[k] = o.real();
        if (!std::isfinite(mission.LapseRanges[0] + mission.LapseRanges[1] + mission.LapseRanges[2]))
          throw Runtime("--lapse-ranges=R0,RA,RB: the distances must be finite.");
        mission.LapseCompanion = "--lapse-ranges";
        break;
      case OPTX_LAPSE_ARRAY:
        mission.LapseArray[0] = o.integer();
        mission.LapseArray[1] = o.integer();
        if (mission.LapseArray[0] < 0 || mission.LapseArray[1] < mission.LapseArray[0])
          throw Runtime("--lapse-array=FIRST,LAST: seismometer indices with 0 <= FIRST <= LAST.");
        mission.LapseCompanion = "--lapse-array";
        break;
      case OPTX_TTIMAGE: {
        if (o.has()) {
          mission.TTGamma = o.real();
          mission.TTNorm = o.real();
        }
        if (mission.TTGamma != 1.0 && mission.TTGamma != 2.0 && mission.TTGamma != 4.0)
          throw Runtime("--ttimage[=GAMMA,NORM]: GAMMA must be 1, 2 or 4 (the gamma root is taken as repeated square roots).");
        if (!(mission.TTNorm >= 0.0 && mission.TTNorm <= 1.0))
          throw Runtime("--ttimage[=GAMMA,NORM]: the norm ratio NORM must lie in [0, 1] (0: by area, 1: by peak).");
        mission.bTTImage = true;
        break;
      }
      case OPTX_TTIMAGE_ARRAY:
        mission.TTArray[0] = o.integer();
        mission.TTArray[1] = o.integer();
        if (mission.TTArray[0] < 0 || mission.TTArray[1] < mission.TTArray[0])
          throw Runtime("--ttimage-array=FIRST,LAST: seismometer indices with 0 <= FIRST <= LAST.");
        mission.TTCompanion = "--ttimage-array";
        break;
      case OPTX_TTIMAGE_AXES:
        for (int k = 0; k < 3; k++) mission.TTAxes[k] = o.real();
        for (int k = 0; k < 3; k++)
          if (!std::isfinite(mission.TTAxes[k]) || mission.TTAxes[k] < 0)
            throw Runtime("--ttimage-axes=X,Y,Z: the weights must be finite and not negative (roots are taken of the weighted energy).");
        mission.TTCompanion = "--ttimage-axes";
        break;
      case OPTX_TTIMAGE_FIT:
        mission.TTFit[0] = o.integer();
        mission.TTFit[1] = o.integer();
        if (mission.TTFit[0] < 1 || mission.TTFit[1] <= mission.TTFit[0])
          throw Runtime("--ttimage-fit=IBEGIN,IEND: the 1-based inclusive points of the array the power law is fitted over, "
                        "1 <= IBEGIN < IEND.");
        mission.TTCompanion = "--ttimage-fit";
        break;
      case OPTX_TTIMAGE_NORMCURVE:
        mission.TTNormCurve[0] = o.real();
        mission.TTNormCurve[1] = o.real();
        if (!(mission.TTNormCurve[0] > 0) || !std::isfinite(mission.TTNormCurve[0]) || !std::isfinite(mission.TTNormCurve[1]))
          throw Runtime("--ttimage-normcurve=C,Q: the curve C X^Q needs C > 0 and both numbers finite.");
        mission.bTTNormCurve = true;
        mission.TTCompanion = "--ttimage-normcurve";
        break;
      case OPTX_TARGET: {
        mission.TargetRel = o.real();
        if (o.has()) mission.TargetCoverage = o.real();
        const long c = o.has() ? o.integer() : (long)mission.TargetMinCount;
        const long r = o.has() ? o.integer() : (long)mission.TargetRounds;
        if (!(mission.TargetRel > 0) || !std::isfinite(mission.TargetRel))
          throw Runtime("--target-error=REL[,COVERAGE[,MINCOUNT[,ROUNDS]]]: REL, the relative standard error aimed at, must be "
                        "finite and > 0.");
        if (!(mission.TargetCoverage > 0 && mission.TargetCoverage <= 1))
          throw Runtime("--target-error=REL[,COVERAGE[,MINCOUNT[,ROUNDS]]]: COVERAGE, the share of the judged entries that must "
                        "meet REL, must lie in (0, 1].");
        if (c < 0)
          throw Runtime("--target-error=REL[,COVERAGE[,MINCOUNT[,ROUNDS]]]: MINCOUNT, the arrivals a bin needs to be judged, must "
                        "not be negative (got " + std::to_string(c) + ").");
        if (r < 1 || r > 64)
          throw Runtime("--target-error=REL[,COVERAGE[,MINCOUNT[,ROUNDS]]]: ROUNDS must be 1 .. 64 (got " + std::to_string(r) + ").");
        mission.TargetMinCount = (unsigned long)c, mission.TargetRounds = (unsigned)r;
        mission.bTarget = true;
        break;
      }
      case OPTX_TARGET_ARRAY:
        mission.TargetArray[0] = o.integer();
        mission.TargetArray[1] = o.integer();
        if (mission.TargetArray[0] < 0 || mission.TargetArray[1] < mission.TargetArray[0])
          throw Runtime("--target-array=FIRST,LAST: seismometer indices with 0 <= FIRST <= LAST.");
        mission.TargetCompanion = "--target-array";
        break;
      case OPTX_TARGET_COMPONENTS: {
        const std::string letters = o.text();
        unsigned mask = 0;
        for (char ch : letters) {
          const size_t k = std::string("XYZPS").find(ch);
          if (k == std::string::npos)
            throw Runtime("--target-components=LETTERS: letters of XYZPS, the energy components that are judged (got '" + letters +
                          "').");
          mask |= 1u << k;
        }
        if (!mask) throw Runtime("--target-components=LETTERS: at least one letter of XYZPS.");
        mission.TargetMask = mask;
        mission.TargetCompanion = "--target-components";
        break;
      }
      case OPTX_ENVSHAPE: {
        long smooth = (long)mission.EnvSmooth;
        if (o.has()) {
          for (int k = 0; k < 2; k++) mission.EnvEdge[k] = o.real();
          for (int k = 0; k < 2; k++) mission.EnvWindow[k] = o.real();
          if (o.has()) smooth = o.integer();
        }
        const double* w = mission.EnvWindow;
        if (!(mission.EnvEdge[0] > 0) || !std::isfinite(mission.EnvEdge[0]) || !std::isfinite(mission.EnvEdge[1]) ||
            !std::isfinite(w[0]) || (!std::isnan(w[1]) && (!std::isfinite(w[1]) || !(w[1] >= w[0]))))
          throw Runtime("--envelope-shape[=V,T0,O,E[,SMOOTH]]: the phase velocity V must be positive, the window's end E not "
                        "before its start O, and every number finite.");
        if (smooth < 0 || smooth > 64)
          throw Runtime("--envelope-shape[=V,T0,O,E[,SMOOTH]]: SMOOTH, the three-point smoothing passes, must be 0 .. 64 (got " +
                        std::to_string(smooth) + ").");
        mission.EnvSmooth = (unsigned)smooth;
        mission.bEnvShape = true;
        break;
      }
      case OPTX_ENVSHAPE_ARRAY:
        mission.EnvArray[0] = o.integer();
        mission.EnvArray[1] = o.integer();
        if (mission.EnvArray[0] < 0 || mission.EnvArray[1] < mission.EnvArray[0])
          throw Runtime("--envelope-array=FIRST,LAST: seismometer indices with 0 <= FIRST <= LAST.");
        mission.EnvCompanion = "--envelope-array";
        break;
      case OPTX_ENVSHAPE_AXES:
        for (int k = 0; k < 3; k++) mission.EnvAxes[k] = o.real();
        for (int k = 0; k < 3; k++)
          if (!std::isfinite(mission.EnvAxes[k]) || mission.EnvAxes[k] < 0)
            throw Runtime("--envelope-axes=X,Y,Z: the weights must be finite and not negative (the envelope's energies must not be).");
        mission.EnvCompanion = "--envelope-axes";
        break;
      case OPTX_ENVFIT: {
        static const char* const form = "--envelope-fit=FILE[,V,T0,O,E[,SMOOTH[,OBSSMOOTH[,MAXLAG_SECONDS]]]]: ";
        mission.FitFile = o.text();
        long smooth = (long)mission.FitSmooth, obs_smooth = (long)mission.FitObsSmooth;
        if (o.has()) {
          for (int k = 0; k < 2; k++) mission.FitEdge[k] = o.real();
          for (int k = 0; k < 2; k++) mission.FitWindow[k] = o.real();
          if (o.has()) smooth = o.integer();
          if (o.has()) obs_smooth = o.integer();
          if (o.has()) mission.FitMaxLagSeconds = o.real();
        }
        const double* w = mission.FitWindow;
        if (mission.FitFile.empty()) throw Runtime(std::string(form) + "FILE, the observed envelopes, must be named.");
        if (!(mission.FitEdge[0] > 0) || !std::isfinite(mission.FitEdge[0]) || !std::isfinite(mission.FitEdge[1]) ||
            !std::isfinite(w[0]) || (!std::isnan(w[1]) && (!std::isfinite(w[1]) || !(w[1] >= w[0]))))
          throw Runtime(std::string(form) + "the phase velocity V must be positive, the window's end E not before its start O, "
                        "and every number finite.");
        if (smooth < 0 || smooth > 64 || obs_smooth < 0 || obs_smooth > 64)
          throw Runtime(std::string(form) + "SMOOTH and OBSSMOOTH, the three-point smoothing passes over the synthetic and the "
                        "observed envelope, must be 0 .. 64 (got " + std::to_string(smooth) + " and " + std::to_string(obs_smooth) + ").");
        if (!(mission.FitMaxLagSeconds >= 0) || !std::isfinite(mission.FitMaxLagSeconds))
          throw Runtime(std::string(form) + "MAXLAG_SECONDS, the largest lag that is tried, must be finite and not negative.");
        mission.FitSmooth = (unsigned)smooth, mission.FitObsSmooth = (unsigned)obs_smooth;
        mission.bEnvFit = true;
        break;
      }
      case OPTX_ENVFIT_ARRAY:
        mission.FitArray[0] = o.integer();
        mission.FitArray[1] = o.integer();
        if (mission.FitArray[0] < 0 || mission.FitArray[1] < mission.FitArray[0])
          throw Runtime("--envelope-fit-array=FIRST,LAST: seismometer indices with 0 <= FIRST <= LAST.");
        mission.FitCompanion = "--envelope-fit-array";
        break;
      case OPTX_ENVFIT_AXES:
        for (int k = 0; k < 3; k++) mission.FitAxes[k] = o.real();
        for (int k = 0; k < 3; k++)
          if (!std::isfinite(mission.FitAxes[k]) || mission.FitAxes[k] < 0)
            throw Runtime("--envelope-fit-axes=X,Y,Z: the weights must be finite and not negative (roots are taken of the weighted energy).");
        mission.FitCompanion = "--envelope-fit-axes";
        break;
      case OPTX_ENVFIT_ENERGY:
        mission.bEnvFitEnergy = true;
        mission.FitCompanion = "--envelope-fit-energy";
        break;
      case OPTX_SLANT: {
        static const char* const form = "--slant-stack=PMIN,PMAX,NP[,RREF[,SMOOTH]]: ";
        for (int k = 0; k < 2; k++) mission.SlantP[k] = o.real();
        const long np = o.integer();
        long smooth = 0;
        if (o.has()) mission.SlantRef = o.real();
        if (o.has()) smooth = o.integer();
        if (!std::isfinite(mission.SlantP[0]) || !std::isfinite(mission.SlantP[1]) || !(mission.SlantP[1] >= mission.SlantP[0]))
          throw Runtime(std::string(form) + "the slownesses (s/km) must be finite, PMAX not below PMIN.");
        if (np < 1 || np > 256 || (np == 1 && mission.SlantP[1] != mission.SlantP[0]))
          throw Runtime(std::string(form) + "NP, the number of slownesses, must be 1 .. 256, and 1 only with PMAX = PMIN (got " +
                        std::to_string(np) + ").");
        if (!std::isnan(mission.SlantRef) && (!std::isfinite(mission.SlantRef) || !(mission.SlantRef > 0)))
          throw Runtime(std::string(form) + "RREF, the reference distance (km), must be finite and positive.");
        if (smooth < 0 || smooth > 64)
          throw Runtime(std::string(form) + "SMOOTH, the three-point smoothing passes, must be 0 .. 64 (got " + std::to_string(smooth) + ").");
        mission.SlantNP = (unsigned)np, mission.SlantSmooth = (unsigned)smooth;
        mission.bSlant = true;
        break;
      }
      case OPTX_SLANT_ARRAY:
        mission.SlantArray[0] = o.integer();
        mission.SlantArray[1] = o.integer();
        if (mission.SlantArray[0] < 0 || mission.SlantArray[1] < mission.SlantArray[0])
          throw Runtime("--slant-array=FIRST,LAST: seismometer indices with 0 <= FIRST <= LAST.");
        mission.SlantCompanion = "--slant-array";
        break;
      case OPTX_SLANT_AXES:
        for (int k = 0; k < 3; k++) mission.SlantAxes[k] = o.real();
        for (int k = 0; k < 3; k++)
          if (!std::isfinite(mission.SlantAxes[k]) || mission.SlantAxes[k] < 0)
            throw Runtime("--slant-axes=X,Y,Z: the weights must be finite and not negative (roots are taken of the weighted energy).");
        mission.SlantCompanion = "--slant-axes";
        break;
      case OPTX_SLANT_ENERGY:
        mission.bSlantEnergy = true;
        mission.SlantCompanion = "--slant-energy";
        break;
      case OPTX_SLANT_RANGEPOWER:
        mission.SlantRangePower = o.real();
        if (!std::isfinite(mission.SlantRangePower)) throw Runtime("--slant-range-power=Q: the exponent of r / r_ref must be finite.");
        mission.SlantCompanion = "--slant-range-power";
        break;
      case OPTX_SLANT_WINDOWS:
        mission.SlantWindows.clear();
        while (o.has()) mission.SlantWindows.push_back(o.real());
        if (mission.SlantWindows.empty() || mission.SlantWindows.size() % 2 || mission.SlantWindows.size() > 16)
          throw Runtime("--slant-windows=T0,T1[,T0,T1...]: one to eight pairs of times in seconds.");
        for (size_t k = 0; k < mission.SlantWindows.size(); k += 2)
          if (!std::isfinite(mission.SlantWindows[k]) || !std::isfinite(mission.SlantWindows[k + 1]) ||
              !(mission.SlantWindows[k + 1] >= mission.SlantWindows[k]))
            throw Runtime("--slant-windows=T0,T1[,T0,T1...]: every time must be finite and no window's end before its start.");
        mission.SlantCompanion = "--slant-windows";
        break;
      case OPTX_CONTRAST: {
        long smooth = 8;
        if (o.has()) smooth = o.integer();
        if (smooth < 0 || smooth > 64)
          throw Runtime("--array-contrast[=SMOOTH]: SMOOTH, the three-point smoothing passes, must be 0 .. 64 (got " + std::to_string(smooth) + ").");
        mission.ContrastSmooth = (unsigned)smooth;
        mission.bContrast = true;
        break;
      }
      case OPTX_CONTRAST_ARGS:
        mission.ContrastArgs.clear();
        while (o.has()) mission.ContrastArgs.push_back(o.real());
        mission.bContrastArgs = true;
        break;
      case OPTX_CONTRAST_ARRAY:
        mission.ContrastArray[0] = o.integer();
        mission.ContrastArray[1] = o.integer();
        if (mission.ContrastArray[0] < 0 || mission.ContrastArray[1] < mission.ContrastArray[0])
          throw Runtime("--contrast-array=FIRST,LAST: seismometer indices with 0 <= FIRST <= LAST.");
        mission.ContrastCompanion = "--contrast-array";
        break;
      case OPTX_CONTRAST_AXES:
        for (int k = 0; k < 3; k++) mission.ContrastAxes[k] = o.real();
        for (int k = 0; k < 3; k++)
          if (!std::isfinite(mission.ContrastAxes[k]) || mission.ContrastAxes[k] < 0)
            throw Runtime("--contrast-axes=X,Y,Z: the weights must be finite and not negative (the rounding bounds need non-negative terms).");
        mission.ContrastCompanion = "--contrast-axes";
        break;
      case OPTX_CONTRAST_WINDOWS:
        mission.ContrastWindows.clear();
        while (o.has()) mission.ContrastWindows.push_back(o.real());
        if (mission.ContrastWindows.empty() || mission.ContrastWindows.size() % 2 || mission.ContrastWindows.size() > 16)
          throw Runtime("--contrast-windows=V1,V2[,V1,V2...]: one to eight pairs of group velocities in km/s.");
        for (size_t k = 0; k < mission.ContrastWindows.size(); k += 2)
          if (!std::isfinite(mission.ContrastWindows[k]) || !(mission.ContrastWindows[k + 1] > 0) ||
              !(mission.ContrastWindows[k] > mission.ContrastWindows[k + 1]))
            throw Runtime("--contrast-windows=V1,V2[,V1,V2...]: every pair must be finite with V1 > V2 > 0 (the window is [r / V1, r / V2]).");
        mission.ContrastCompanion = "--contrast-windows";
        break;
      case OPTX_CONTRAST_REGIONS:
        mission.ContrastRegions.clear();
        while (o.has()) mission.ContrastRegions.push_back(o.real());
        if (mission.ContrastRegions.empty() || mission.ContrastRegions.size() % 2 || mission.ContrastRegions.size() > 16)
          throw Runtime("--contrast-regions=R0,R1[,R0,R1...]: one to eight pairs of distances in km.");
        for (size_t k = 0; k < mission.ContrastRegions.size(); k += 2)
          if (!std::isfinite(mission.ContrastRegions[k]) || !std::isfinite(mission.ContrastRegions[k + 1]) ||
              !(mission.ContrastRegions[k + 1] >= mission.ContrastRegions[k]))
            throw Runtime("--contrast-regions=R0,R1[,R0,R1...]: every distance must be finite and no region's end before its start.");
        mission.ContrastCompanion = "--contrast-regions";
        break;
      case OPTX_CONTRAST_RANGEPOWER:
        mission.ContrastRangePower = o.real();
        if (!std::isfinite(mission.ContrastRangePower)) throw Runtime("--contrast-range-power=Q: the exponent of r / r_ref must be finite.");
        mission.ContrastCompanion = "--contrast-range-power";
        break;
      case OPTX_CONTRAST_SEED:
        mission.ContrastSeed = (unsigned long)std::strtoull(o.text().c_str(), nullptr, 0);
        mission.bContrastSeed = true;
        mission.ContrastCompanion = "--contrast-seed";
        break;
      case OPTX_CONTRAST_NUMBER:
        mission.ContrastNumPhonons = o.integer();
        if (mission.ContrastNumPhonons < 0) throw Runtime("--contrast-num-phonons=N: the test run's histories cannot be negative.");
        mission.ContrastCompanion = "--contrast-num-phonons";
        break;
      case OPTX_BANDS: {
        static const char* const form = "--envelope-bands=R,LEVEL[,V,T0,O,E[,SMOOTH]]: ";
        const long replicates = o.integer();
        mission.BandsLevel = o.real();
        long smooth = (long)mission.BandsSmooth;
        if (o.has()) {
          for (int k = 0; k < 2; k++) mission.BandsEdge[k] = o.real();
          for (int k = 0; k < 2; k++) mission.BandsWindow[k] = o.real();
          if (o.has()) smooth = o.integer();
        }
        if (replicates < 1 || replicates > 4096)
          throw Runtime(std::string(form) + "R, the resamples of the batches, must be 1 .. 4096 (got " + std::to_string(replicates) + ").");
        if (!(mission.BandsLevel > 0 && mission.BandsLevel < 1))
          throw Runtime(std::string(form) + "LEVEL, the share of the replicates between the bands, must lie in (0, 1).");
        const double tail = std::floor((0.5 * (1.0 - mission.BandsLevel)) * (double)replicates);
        if (2 * tail >= (double)replicates)
          throw Runtime(std::string(form) + "the tail floor((0.5 (1 - LEVEL)) R) = " + std::to_string((long)tail) +
                        " leaves nothing between the bands of " + std::to_string(replicates) + " replicates.");
        const double* w = mission.BandsWindow;
        if (!(mission.BandsEdge[0] > 0) || !std::isfinite(mission.BandsEdge[0]) || !std::isfinite(mission.BandsEdge[1]) ||
            !std::isfinite(w[0]) || (!std::isnan(w[1]) && (!std::isfinite(w[1]) || !(w[1] >= w[0]))))
          throw Runtime(std::string(form) + "the phase velocity V must be positive, the window's end E not before its start O, and "
                        "every number finite.");
        if (smooth < 0 || smooth > 64)
          throw Runtime(std::string(form) + "SMOOTH, the three-point smoothing passes, must be 0 .. 64 (got " + std::to_string(smooth) +
                        ").");
        mission.BandsReplicates = (unsigned)replicates, mission.BandsTail = (unsigned)tail, mission.BandsSmooth = (unsigned)smooth;
        mission.bBands = true;
        break;
      }
      case OPTX_BANDS_ARRAY:
        mission.BandsArray[0] = o.integer();
        mission.BandsArray[1] = o.integer();
        if (mission.BandsArray[0] < 0 || mission.BandsArray[1] < mission.BandsArray[0])
          throw Runtime("--bands-array=FIRST,LAST: seismometer indices with 0 <= FIRST <= LAST.");
        mission.BandsCompanion = "--bands-array";
        break;
      case OPTX_BANDS_AXES:
        for (int k = 0; k < 3; k++) mission.BandsAxes[k] = o.real();
        for (int k = 0; k < 3; k++)
          if (!std::isfinite(mission.BandsAxes[k]) || mission.BandsAxes[k] < 0)
            throw Runtime("--bands-axes=X,Y,Z: the weights must be finite and not negative (the envelope's energies must not be).");
        mission.BandsCompanion = "--bands-axes";
        break;
      case OPTX_BANDS_SEED:
        mission.BandsSeed = (unsigned long)std::strtoull(o.text().c_str(), nullptr, 0);
        mission.BandsCompanion = "--bands-seed";
        break;
      case OPTX_DEVTABLES: par.DeviceTables = true; break;
      case OPTX_HOSTTABLES: par.HostTables = true, par.DeviceTables = false; break;
    }
  }
  // --job-error-batches=N deals the job's N batches evenly to the shards that --gpus / --devices name
  if (mission.JobErrorBatches) {
    const unsigned long shards = shard_count(mission);
    const unsigned long N = mission.JobErrorBatches;
    const std::string over = std::to_string(N) + " batches over " + std::to_string(shards) + (shards == 1 ? " shard" : " shards");
    if (mission.ErrorBatches)
      throw Runtime("--job-error-batches cannot be combined with --error-batches: the first cuts the whole job into its N "
                    "batches, the second one device's share into B.");
    if (ReportMaskFromKeywords(mission.Reports))
      throw Runtime("--job-error-batches cannot be combined with --reports (the event log's launches run one at a time).");
    if (N % shards)
      throw Runtime("--job-error-batches=N: N must be a multiple of the number of shards (got " + over + ").");
    if (N / shards < 2 || N / shards > 64)
      throw Runtime("--job-error-batches=N: every shard runs N / shards batches, which must be 2 .. 64 (got " + over + ").");
  }
  // the batched products (batch_products.hpp), in the order of the table: each is made where ONE device's batch blocks lie
  // and keeps them for itself.  The first rule that is broken speaks
  const std::string each_keeps = " in one run (each keeps the run's batch blocks for itself): out of scope.";
  for (const BatchProduct& p : kBatchProducts) {
    const std::string option = p.option;
    if (mission.*p.companion && !(mission.*p.given))
      throw Runtime(std::string(mission.*p.companion) + " needs " + option + ": it only says " + p.only_says + ".");
    if (p.kind == BatchKind::CONTRAST && mission.bContrastArgs && !mission.bContrast)
      throw Runtime("--contrast-model-args needs --array-contrast: it names the model the command line's own is compared with.");
    if (!(mission.*p.given)) continue;
    if (p.kind == BatchKind::CONTRAST && !mission.bContrastArgs)
      throw Runtime("--array-contrast needs --contrast-model-args=a,b,...: the arguments of the test model, which the command "
                    "line's own model (the base) is compared with.");
    if (mission.JobErrorBatches)
      throw Runtime(option + " cannot be combined with --job-error-batches: " + p.made_where + " (" + p.call + ")" +
                    (p.call_noun ? std::string("; a job sharded over devices has no ") + p.call_noun + " call" : std::string()) +
                    ".  Use --error-batches=B.");
    if (!mission.ErrorBatches) throw Runtime(option + " needs --error-batches=B: " + p.needs_batches);
    // (every earlier product in the table's order: where --target-error and a product behind it stand before this one, that
    //  product's own turn has refused the two already, so the rounds' sentence never hides another)
    for (const BatchProduct* q = kBatchProducts; q != &p; q++) {
      if (!(mission.*q->given)) continue;
      const char* blocks = p.needs_blocks && q->needs_blocks ? nullptr : p.needs_blocks ? p.needs_blocks : q->needs_blocks;
      throw Runtime(option + " cannot be combined with " + q->option +
                    (blocks ? " (" + std::string(blocks) + ", the rounds keep only their moments): out of scope." : each_keeps));
    }
    if (p.refuses_reports && ReportMaskFromKeywords(mission.Reports))
      throw Runtime(option + " cannot be combined with --reports (the event log's launches run one at a time).");
    if (p.one_device && shard_count(mission) > 1)
      throw Runtime(option + " runs on one device: --gpus / --devices name " + std::to_string(shard_count(mission)) + " shards (" +
                    p.one_device + ").");
    // what is one product's own
    if (p.kind == BatchKind::IMAGE && mission.bTTNormCurve && mission.TTFit[0] == 0)
      throw Runtime("--ttimage-normcurve needs --ttimage-fit=IBEGIN,IEND: the curve's range window comes from the fit's array.");
    if (p.kind == BatchKind::PRECISION) {
      const long n = par.NumPhonons, R = (long)mission.TargetRounds;
      if (n < 0 || n % R)
        throw Runtime("--target-error: --num-phonons (" + std::to_string(n) + "), the cap, must be a multiple of ROUNDS (" +
                      std::to_string(R) + "): every round runs the same number of histories.");
      if (n / R < (long)mission.ErrorBatches)
        throw Runtime("--target-error: a round of --num-phonons / ROUNDS = " + std::to_string(n / R) + " histories is fewer than the " +
                      std::to_string(mission.ErrorBatches) + " batches of --error-batches.");
    }
    if (p.kind == BatchKind::CONTRAST) {
      if (!mission.ContrastRegions.empty() && mission.ContrastWindows.empty())
        throw Runtime("--contrast-regions needs --contrast-windows: a region's sums are sums of window energies.");
      const long n_test = mission.ContrastNumPhonons < 0 ? par.NumPhonons : mission.ContrastNumPhonons;
      if (n_test < (long)mission.ErrorBatches)
        throw Runtime("--array-contrast: the test run's " + std::to_string(n_test) + " histories are fewer than the " +
                      std::to_string(mission.ErrorBatches) + " batches of --error-batches.");
    }
  }
  // the views and the maps are made from the grid: none of their options means anything without it
  if (!mission.bScatterGrid && (mission.bScatterViews || mission.bViewAzimuth || mission.bNoScatterGridFile || mission.bScatterMaps))
    throw Runtime(std::string(mission.bScatterViews ? "--scatter-views" : mission.bViewAzimuth ? "--scatter-view-azimuth"
                              : mission.bNoScatterGridFile ? "--no-scatter-grid-file" : "--scatter-maps") +
                  " needs --scatter-grid: the views (--scatter-views, --scatter-view-azimuth, --no-scatter-grid-file) and the "
                  "maps (--scatter-maps) are made from that grid.");
  if (mission.bNoScatterGridFile && !mission.bScatterViews)
    throw Runtime("--no-scatter-grid-file needs --scatter-views: without the views the run would leave nothing of its grid.");
  if (mission.bViewAzimuth && !mission.bScatterViews)
    throw Runtime("--scatter-view-azimuth needs --scatter-views: it filters the elevation view.");
}
