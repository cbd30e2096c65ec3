// batch_out.hpp -- the batched-run stage of ./main: what --error-batches, --job-error-batches and the batched products of
// batch_products.hpp (--lapse-windows, --ttimage, --target-error, --envelope-shape, --envelope-fit, --slant-stack,
// --array-contrast) run in place of the plain run, and what they write after it (seis_NNN_err.octv, then the product's file:
// lapse.octv, ttimage.octv, precision.octv, envshape.octv, envfit.octv, slantstack.octv, contrast.octv, envbands.octv).
// Compiled into ./main beside main.cpp (it calls r3d_run_batched* and r3d_node_run_batched of the engine's library, so
// it is no part of libr3d_host.so); its row arithmetic is batch_plan.hpp.
#ifndef R3DH_BATCH_OUT_HPP_
#define R3DH_BATCH_OUT_HPP_

#include <memory>
#include <ostream>
#include <string>
#include <vector>

#include "../../include/r3d.h"
#include "../../include/r3d_host.h"
#include "batch_products.hpp"
#include "model.hpp"

// A file of the run: `name` under --output-dir ("" = the current directory).
inline std::string output_path(const std::string& dir, const std::string& name) { return dir.empty() ? name : dir + "/" + name; }

// What the options ask for, where it goes, and -- after the run -- every bin's standard error.  As it stands here it is the
// job of the plain kinds (NONE, ERRORS, JOB_ERRORS); every product of batch_products.hpp is a type of its own in
// batch_out.cpp that is made with its plan, overrides run() and write() and keeps what its run made for its file.
struct BatchJob {
  BatchKind kind = BatchKind::NONE;
  unsigned batches = 0;       // (PRECISION: of a round)
  unsigned batches_run = 0;   // after run(): the batches the standard errors come from (PRECISION: those of the rounds run)
  std::string dir;            // --output-dir
  std::vector<double> energy_se, counts_se;
  virtual ~BatchJob() = default;
  // The run of the ids 0 .. n - 1 in the job's batches into `total`, energy_se and counts_se (sized by the caller).  Here:
  // the whole job as N batches dealt to the shards, every shard's moments taken on its device and merged on shard 0's
  // (JOB_ERRORS: include/r3d.h r3d_node_run_batched), or the one shard's ids as B batches, every bin's standard error from
  // their spread (ERRORS: r3d_run_batched); the totals are those of the plain run up to summation order.
  virtual void run(const r3d_model_desc& model, r3d_node* node, uint64_t n, uint64_t seed, r3d_result& total);
  // The product's file (the plain kinds have none).
  virtual void write(const Model&, std::ostream&) const {}
};

// The job of a simulation run (`kind` stays NONE without one of the options).  The model is needed for the arrays: throws
// what the product's Request and Plan (dataout.hpp: LapseRequest / LapsePlan ... ContrastRequest / ContrastPlan) throw.
// `par`: what the model was built from -- --array-contrast builds its test model from it here, on the host, and refuses one
// whose seismometers or bins differ.
std::unique_ptr<BatchJob> make_batch_job(const MissionParams& mission, const Model& model, const ModelParams& par);

// What --error-batches cannot be combined with, told BEFORE the node is built.  Throws Runtime.
void check_batch_job(const BatchJob& job, size_t n_shards, uint32_t report_mask);

// The job's run (kind != NONE), on the node's one shard or, for JOB_ERRORS, over all of them: `total` (whose arrays the
// caller owns) gets the sums, the job the rest.  Prints the `|  Batches: ...` line.  Throws Runtime.
void run_batch_job(BatchJob& job, const r3d_model_desc& model, r3d_node* node, uint64_t n, uint64_t seed, r3d_result& total);

// seis_NNN_err.octv, then the product's file, under the job's directory.  Throws Runtime.
void write_batch_outputs(const BatchJob& job, const Model& model);

#endif
