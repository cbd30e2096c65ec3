// batch_products.hpp -- the table of ./main's batched products: the options that run with --error-batches=B, keep the run's
// batch blocks on ONE device for what they make there, and write one .octv file beside seis_NNN_err.octv.  One record per
// product, in the order they were introduced.  cmdline.cpp reads it for what the options rule out (one loop: every product
// against --job-error-batches, a missing --error-batches, every earlier product, --reports, several shards), batch_out.cpp
// for the kind of the run's job and the name of its file.  A new product is a record here, its parse cases, and its type in
// batch_out.cpp.
#ifndef R3DH_BATCH_PRODUCTS_HPP_
#define R3DH_BATCH_PRODUCTS_HPP_

#include "cmdline.hpp"

// What a batched run is.  ERRORS: --error-batches alone; JOB_ERRORS: --job-error-batches; the others: --error-batches with the
// product of that record below.
enum class BatchKind { NONE, ERRORS, LAPSE, IMAGE, JOB_ERRORS, PRECISION, SHAPE, FIT, SLANT, CONTRAST, BANDS };

struct BatchProduct {
  const char* option;
  bool MissionParams::*given;
  const char* MissionParams::*companion;   // one of its companion options that was given (refused without the product)
  BatchKind kind;
  const char* file;                        // under --output-dir
  // the words of the refusals that differ from product to product (cmdline.cpp puts the sentences together)
  const char* only_says;       // "<companion> needs <option>: it only says ...."
  const char* made_where;      // "<option> cannot be combined with --job-error-batches: ... (<call>)"
  const char* call;            //   the entry of include/r3d.h that makes it
  const char* call_noun;       //   "; a job sharded over devices has no ... call" (null: the sentence ends at the call)
  const char* needs_batches;   // "<option> needs --error-batches=B: ..."
  const char* needs_blocks;    // with --target-error: "(..., the rounds keep only their moments)" (null: --target-error itself)
  // the checks that not every product makes when the options are read
  bool refuses_reports;        // (--lapse-windows and --ttimage leave --reports to check_batch_job, batch_out.hpp)
  const char* one_device;      // null, or why several shards are refused here already: "<option> runs on one device: ... (...)"
};

inline const BatchProduct kBatchProducts[] = {
    {"--lapse-windows", &MissionParams::bLapse, &MissionParams::LapseCompanion, BatchKind::LAPSE, "lapse.octv",
     "how those windows are summed", "the window sums are taken where ONE device's batch blocks lie", "r3d_run_batched_windows",
     "windows", "the windows' standard errors and the ratios' jackknife come from the B batches.",
     "the window sums need one run's batch blocks", false, nullptr},
    {"--ttimage", &MissionParams::bTTImage, &MissionParams::TTCompanion, BatchKind::IMAGE, "ttimage.octv",
     "how that image is made", "the image is made where ONE device's batch blocks lie", "r3d_run_batched_array_image", "image",
     "the pixels' and the fit's standard errors are jackknives over the B batches.", "the image needs one run's batch blocks", false,
     nullptr},
    {"--target-error", &MissionParams::bTarget, &MissionParams::TargetCompanion, BatchKind::PRECISION, "precision.octv",
     "which entries are judged", "the rounds are judged where ONE device's batch blocks lie", "r3d_run_to_precision", nullptr,
     "every round runs as B batches, and the standard errors that are judged come from the batches of all rounds so far.", nullptr,
     true, "a run in rounds over several devices is not built"},
    {"--envelope-shape", &MissionParams::bEnvShape, &MissionParams::EnvCompanion, BatchKind::SHAPE, "envshape.octv",
     "how that shape is made", "the shape is made where ONE device's batch blocks lie", "r3d_run_batched_envelope_shape", "shape",
     "the standard errors of the shape's numbers are jackknives over the B batches.", "the shape needs one run's batch blocks", true,
     nullptr},
    {"--envelope-fit", &MissionParams::bEnvFit, &MissionParams::FitCompanion, BatchKind::FIT, "envfit.octv",
     "how that misfit is made", "the misfit is made where ONE device's batch blocks lie", "r3d_run_batched_envelope_misfit", "misfit",
     "the standard errors of the misfit's numbers are jackknives over the B batches.", "the misfit needs one run's batch blocks", true,
     nullptr},
    {"--slant-stack", &MissionParams::bSlant, &MissionParams::SlantCompanion, BatchKind::SLANT, "slantstack.octv",
     "how that stack is made", "the stack is made where ONE device's batch blocks lie", "r3d_run_batched_slant_stack", "slant",
     "the standard errors of the stack, the power and the picks are jackknives over the B batches.",
     "the stack needs one run's batch blocks", true, nullptr},
    {"--array-contrast", &MissionParams::bContrast, &MissionParams::ContrastCompanion, BatchKind::CONTRAST, "contrast.octv",
     "how that contrast is made", "the contrast is made where ONE device's batch blocks of both runs lie", "r3d_run_batched_contrast",
     "contrast", "the standard errors of the contrast are two-sample jackknives over the B batches of either run.",
     "the contrast needs both runs' batch blocks", true, "both runs' batch blocks must lie on the same device"},
    {"--envelope-bands", &MissionParams::bBands, &MissionParams::BandsCompanion, BatchKind::BANDS, "envbands.octv",
     "how those bands are made", "the bands are made where ONE device's batch blocks lie", "r3d_run_batched_envelope_bands", "bands",
     "the bands are percentiles over resamples of the B batches.", "the bands need one run's batch blocks", true, nullptr},
};

#endif
