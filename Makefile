# Build of the MI355X phonon-transport engine and its host-side pieces.
#
#   make            every binary the package, ./main and the tests load (default: all of the below)
#   make host       radiative3d_amd/lib/libr3d_host.so   (g++)
#   make engine     radiative3d_amd/lib/libr3d_hip.so    (hipcc, gfx950)
#   make repro      radiative3d_amd/lib/libr3d_hip_repro.so  (the same engine, bit-defined per history)
#   make oracle     oracle/libr3d_oracle.so, oracle/libr3d_tables_oracle.so  (g++; test infrastructure)
#   make cli        ./main                               (g++; the reference's command-line surface)
#   make devtest    tests/emul/libr3d_{physics,tables,collect}_device{,_repro}.so  (hipcc, gfx950; test infrastructure)
#   make emul       tests/emul/libr3d_emul.so            (g++; the kernels' per-lane code on the host, test infrastructure)
#   make stepfinals radiative3d_amd/lib/variant_STEPFINALS.so  (make variant NAME=STEPFINALS ...; test infrastructure)
#   make variant NAME=X DEFS=... [DEFS_CYL= DEFS_TET= DEFS_SPH=]   a developer build of the engine (at the end of this file)
#
# Every engine object -- of the two shipped builds and of any variant -- comes from ONE rule template (engine_object)
# over ONE table of units; parallelism is make's -j everywhere.
# `make -q` succeeding is what scripts/do-fundamentals.sh (reference :145-152)
# checks before a run.

CXX      ?= g++
HIPCC    ?= /opt/rocm/bin/hipcc
CXXFLAGS ?= -std=c++17 -O2 -fPIC -Wall -Wno-unused-function -Wno-unknown-pragmas
# -disable-machine-licm: the kernel is one long loop; hoisting every polynomial constant out of it
# costs ~60 registers (measured with machine-LICM on: 256 registers and 100+ spilled, DESIGN.md
# section 6); without the hoist the three kernels hold 162-167 and fit three waves per SIMD.
# -amdgpu-atomic-optimizer-strategy=None: the kernels' atomics on a uniform address are issued by ONE
# lane already (a batch's tallies, the id counter); the optimiser still wraps each in its generic
# reduction (lane election, a scalar loop over the active lanes): 1-2.5 % of the kernel time.
HIPFLAGS ?= -std=c++17 -O3 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function -Wno-bitwise-instead-of-logical \
            -mllvm -disable-machine-licm -mllvm -amdgpu-atomic-optimizer-strategy=None
# The traversal kernels are one translation unit per cell kind (csrc/r3d_kernels_kind.hip), each with
# the instruction scheduler that suits it: under the compiler's max-ILP strategy the spherical-shell
# kernel runs 3.4 % faster (no vector register spilled, against 4) and the layered one 0.4 %, the
# tetra kernel 1.4 % slower (10 spilled against 4).
HIPFLAGS_CYL ?= -mllvm -amdgpu-sched-strategy=max-ilp
HIPFLAGS_TET ?=
HIPFLAGS_SPH ?= -mllvm -amdgpu-sched-strategy=max-ilp

LIBDIR   := radiative3d_amd/lib
HOSTDIR  := radiative3d_amd/host
CSRC     := radiative3d_amd/csrc
COMMON   := radiative3d_amd/common

HOST_SRC := $(HOSTDIR)/ecs.cpp $(HOSTDIR)/grid.cpp $(HOSTDIR)/model.cpp \
            $(HOSTDIR)/models_builtin.cpp $(HOSTDIR)/cmdline.cpp $(HOSTDIR)/dataout.cpp \
            $(HOSTDIR)/capi.cpp
HOST_HDR := $(wildcard $(HOSTDIR)/*.hpp) include/r3d.h include/r3d_host.h radiative3d_amd/stats/r3d_window_sums.h \
            radiative3d_amd/arrays/r3d_array_image.h $(wildcard radiative3d_amd/shapes/*.h) radiative3d_amd/beams/r3d_slant_stack.h \
            radiative3d_amd/contrasts/r3d_array_contrast.h
ENGINE_HDR := $(wildcard $(CSRC)/*.h) include/r3d.h
# The add-ons: what stands beside the engine on its C-ABI, each a directory radiative3d_amd/<name>/ of ONE .hip and
# its headers, which includes $(COMMON)/r3d_entry.h and include/r3d.h and nothing from csrc/.  A new one is a word here.
#   stats  per-bin standard errors from batches (r3d_batch_moments, r3d_run_device_batched), lapse-window sums (r3d_window_sums)
#   views  the two video views of the scatter-event grid (r3d_volume_project, r3d_volume_range_bins)
#   maps   the grid reduced along its frame axis: arrival-time, peak and total maps (r3d_volume_time_maps)
#   arrays the travel-time image of a receiver array with jackknife errors (r3d_array_image, r3d_run_batched_array_image)
#   precision  a run to a target standard error: the judge kernel and the rounds around it, on top of the stats add-on's
#          C-ABI (r3d_batch_precision, r3d_run_to_precision)
#   shapes the envelope shape per receiver -- peak delay, decay to half, centroid, width -- with jackknife errors
#          (r3d_envelope_shape, r3d_run_batched_envelope_shape)
#   fits   the envelope misfit against observed data -- scale, correlation, residual, lag -- with jackknife errors
#          (r3d_envelope_misfit, r3d_run_batched_envelope_misfit)
#   beams  the slant stack of a receiver array -- the vespagram, the beam power per slowness, the picked slowness and delay per
#          window -- with jackknife errors (r3d_slant_shifts, r3d_slant_stack, r3d_run_batched_slant_stack)
#   contrasts  the contrast of two runs along a receiver array -- per pixel, per window, per region of the array -- with the
#          two-sample jackknife over both runs' batches (r3d_array_contrast, r3d_run_batched_contrast, r3d_contrast_decibel)
#   bands  bootstrap percentile bands of the envelope and its six shape numbers: the batches resampled R times, order
#          statistics per bin and number (r3d_bootstrap_counts, r3d_envelope_bands, r3d_run_batched_envelope_bands)
ADDONS := stats views maps arrays precision shapes fits beams contrasts bands
addon_src = $(wildcard radiative3d_amd/$(1)/*.hip)
# (arrays/ takes the bin energy and the strand constants from stats/r3d_window_sums.h; shapes/ those and the scans, the
# running maximum and the jackknife from arrays/r3d_array_image.h; fits/ all of that and every header of shapes/: the rows
# of a receiver with their smoothing rule, r3d_envelope_rows.h, and the shape's arithmetic; beams/ and contrasts/ the same
# headers as fits/, and so does bands/)
addon_hdr = $(wildcard radiative3d_amd/$(1)/*.h) $(COMMON)/r3d_entry.h include/r3d.h $(if $(filter arrays,$(1)),radiative3d_amd/stats/r3d_window_sums.h) \
            $(if $(filter shapes,$(1)),radiative3d_amd/stats/r3d_window_sums.h radiative3d_amd/arrays/r3d_array_image.h) \
            $(if $(filter fits,$(1)),radiative3d_amd/stats/r3d_window_sums.h radiative3d_amd/arrays/r3d_array_image.h $(wildcard radiative3d_amd/shapes/*.h)) \
            $(if $(filter beams contrasts bands,$(1)),radiative3d_amd/stats/r3d_window_sums.h radiative3d_amd/arrays/r3d_array_image.h $(wildcard radiative3d_amd/shapes/*.h))
OBJDIR   := build/obj

# (the default goal is the first target of the file: it has to come before the generated object rules)
.PHONY: all host engine repro oracle cli devtest emul stepfinals variant clean FORCE
.DELETE_ON_ERROR:
all: host engine repro oracle cli devtest emul stepfinals

# The engine's own units.  The traversal kernels are one source compiled once per cell kind: KIND_<unit> is the name
# the kind's switches carry (HIPFLAGS_<K> above, DEFS_<K> of a variant) and its number.
UNITS      := engine tables volume cyl tet sph
SRC_engine := $(CSRC)/r3d_engine.hip
SRC_tables := $(CSRC)/r3d_tables_build.hip
SRC_volume := $(CSRC)/r3d_volume.hip
$(foreach k,cyl tet sph,$(eval SRC_$(k) := $(CSRC)/r3d_kernels_kind.hip))
HDR_volume := $(COMMON)/r3d_entry.h
KIND_cyl   := CYL 0
KIND_tet   := TET 1
KIND_sph   := SPH 2
# unit_src(unit), unit_hdr(unit): of an engine unit from the table, of an add-on from its directory
unit_src = $(or $(SRC_$(1)),$(call addon_src,$(1)))
unit_hdr = $(if $(SRC_$(1)),$(ENGINE_HDR) $(HDR_$(1)),$(call addon_hdr,$(1)))
# unit_cc(unit, flags of the build): the compile line of one unit up to its -o
unit_cc = $(HIPCC) $(HIPFLAGS) $(HIPFLAGS_$(word 1,$(KIND_$(1)))) $(2) $(addprefix -DR3D_KIND=,$(word 2,$(KIND_$(1)))) -c
# engine_object(tag, unit, flags of the build, further prerequisites): THE rule for an object of any engine build
define engine_object
$(OBJDIR)/$(1)_$(2).o: $(call unit_src,$(2)) $(call unit_hdr,$(2)) $(4)
	@mkdir -p $(OBJDIR)
	$(call unit_cc,$(2),$(3)) -o $$@ $(call unit_src,$(2))

endef
# engine_library(library, tag, units in link order): THE link rule
engine_objs = $(foreach u,$(2),$(OBJDIR)/$(1)_$(u).o)
define engine_library
$(1): $(call engine_objs,$(2),$(3))
	@mkdir -p $(LIBDIR)
	$(HIPCC) --offload-arch=gfx950 -shared -pthread -o $$@ $(call engine_objs,$(2),$(3)) $(RCCL_LIBS)

endef
# (librccl is bound at first use, csrc/r3d_rccl.h: the copy already in the process if there is one)
RCCL_LIBS ?= -ldl

# The two shipped builds: `main` with the flags above, `repro` with two more.  build_suffix(tag) is what a build's libraries
# carry in their names: nothing for main, _repro for repro.
BUILDS      := main repro
FLAGS_repro := -DR3D_REPRODUCIBLE -ffp-contract=off
build_suffix = $(subst _main,,_$(1))
$(foreach b,$(BUILDS),$(foreach u,$(UNITS) $(ADDONS),$(eval $(call engine_object,$(b),$(u),$(FLAGS_$(b))))))
$(foreach b,$(BUILDS),$(eval $(call engine_library,$(LIBDIR)/libr3d_hip$(call build_suffix,$(b)).so,$(b),$(ADDONS) $(UNITS))))

host: $(LIBDIR)/libr3d_host.so
engine: $(LIBDIR)/libr3d_hip.so
# the same engine with every wave-voted series choice taken out (r3d_math.h all_lanes) and no
# contraction of a * b + c into fused multiply-adds beyond the ones the sources spell out (the
# compiler contracts differently in each kernel it inlines the physics into: the diagnostic and the
# production kernels then differ in the last bits, ~1e-10 after an ill-conditioned travel time): a
# history's result is then bit-defined by (model, seed, id) in every kernel; loaded under
# R3D_REPRODUCIBLE=1.  Costs 5-10 %.
repro: $(LIBDIR)/libr3d_hip_repro.so
oracle: oracle/libr3d_oracle.so oracle/libr3d_tables_oracle.so
cli: main

# The command-line program the reference's do-*.sh scripts call as ./main
MAIN_SRC := $(HOSTDIR)/main.cpp $(HOSTDIR)/scatter_out.cpp $(HOSTDIR)/batch_out.cpp
main: $(MAIN_SRC) $(HOSTDIR)/scatter_out.hpp $(HOSTDIR)/scatter_plan.hpp $(HOSTDIR)/batch_out.hpp $(HOSTDIR)/batch_plan.hpp $(HOSTDIR)/batch_products.hpp \
      $(LIBDIR)/libr3d_host.so $(LIBDIR)/libr3d_hip.so $(ENGINE_HDR)
	$(CXX) $(CXXFLAGS) -pthread -o $@ $(MAIN_SRC) -L$(LIBDIR) -lr3d_host -lr3d_hip \
	    -Wl,-rpath,'$$ORIGIN/$(LIBDIR)' -Wl,-rpath,/opt/rocm/lib

$(LIBDIR)/libr3d_host.so: $(HOST_SRC) $(HOST_HDR)
	@mkdir -p $(LIBDIR)
	$(CXX) $(CXXFLAGS) -shared -pthread -o $@ $(HOST_SRC)

oracle/libr3d_oracle.so: oracle/r3d_oracle.cpp oracle/philox.h include/r3d.h
	$(CXX) $(CXXFLAGS) -shared -o $@ oracle/r3d_oracle.cpp

# the table builders restated (take-off set, scatterer tables, source patterns, seismometer axes):
# plain g++, no fast-math, no FMA contraction -- the reference's operation order is the point
oracle/libr3d_tables_oracle.so: oracle/r3d_tables_oracle.cpp
	$(CXX) -std=c++17 -O2 -ffp-contract=off -fPIC -Wall -shared -o $@ oracle/r3d_tables_oracle.cpp

# The per-lane physics case by case on the device (tests/test_physics_device.py): ONE test-only unit outside csrc/,
# which includes the engine's headers and tests/emul/physics_cases.h, compiled with the engine's flags and with the
# reproducible build's -- sibling compilations of the same text, not the traversal kernels' code objects.
# (Its guided draws can take their guide from the engine's build_guide_on_device: the engine's table object is linked in,
# named BEFORE the source on the command line: hipcc reads whatever follows a .hip file as HIP text.)
# The table builders entry by entry (tests/test_tables_build_device.py): thin test-only entries linked with the table
# OBJECTS of the two engine builds -- the code libr3d_hip.so and libr3d_hip_repro.so carry, not a sibling compilation.
# The receiver collection arrival by arrival (tests/test_collect_device.py): a sibling compilation again, of r3d_pool.h's
# pool_collect_pairs, r3d_wave.h and r3d_step.h's collect.
DEVTESTS    := physics tables collect
HDR_physics := tests/emul/physics_cases.h
device_test_lib = tests/emul/libr3d_$(1)_device$(call build_suffix,$(2)).so
# device_test(name, build): tests/emul/<name>_device.hip under the build's flags, with the build's table object
define device_test
$(call device_test_lib,$(1),$(2)): tests/emul/$(1)_device.hip $(HDR_$(1)) $(ENGINE_HDR) $(OBJDIR)/$(2)_tables.o
	$(HIPCC) $(HIPFLAGS) $(FLAGS_$(2)) -shared -o $$@ $(OBJDIR)/$(2)_tables.o tests/emul/$(1)_device.hip

endef
$(foreach t,$(DEVTESTS),$(foreach b,$(BUILDS),$(eval $(call device_test,$(t),$(b)))))
devtest: $(foreach t,$(DEVTESTS),$(foreach b,$(BUILDS),$(call device_test_lib,$(t),$(b))))

# The kernels' per-lane code built for the host (tests/emul_ffi.py, tests/emul/emul.cpp: it includes csrc/'s headers)
emul: tests/emul/libr3d_emul.so
tests/emul/libr3d_emul.so: tests/emul/emul.cpp tests/emul/physics_cases.h $(ENGINE_HDR)
	$(CXX) -std=c++17 -O2 -fPIC -shared -o $@ tests/emul/emul.cpp

# A test-only sibling compilation of the engine: the chain-step kernel with its final-record stores compiled in
# (tests/test_gpu_parity.py holds it per history against the oracle; never loaded by the product)
stepfinals:
	$(MAKE) variant NAME=STEPFINALS DEFS=-DR3D_STEP_FINALS=1

clean:
	rm -f $(LIBDIR)/*.so oracle/*.so tests/emul/*.so main
	rm -rf $(OBJDIR)

# Developer variants of the engine (timing-only / diagnostic builds, never shipped as libr3d_hip.so;
# the only builds that say -DR3D_DEV_BUILD, without which the R3D_ABLATE_* / R3D_PHASE_TIMING switches
# are a compile error -- csrc/r3d_tables.h):
#   make -j8 variant NAME=PHASE DEFS="-DR3D_PHASE_TIMING"   ->  radiative3d_amd/lib/variant_PHASE.so
# run through the tools with R3D_HIP_LIB=radiative3d_amd/lib/variant_PHASE.so (tools/time_chain.py,
# tools/pool_stats.py pass it to Engine(lib=...); the library itself reads no environment).
# The objects are engine_object's, tagged v$(NAME), each with a prerequisite more: a stamp that holds its compile line and
# is rewritten only when that line changes.  So a changed switch recompiles the units it reaches and no other, and
# the library is never linked from an object compiled under other flags.  Nor from one a failed compile left behind:
# the library is removed before anything is brought up to date, and linked again only after every object is.
VDEFS = -DR3D_DEV_BUILD $(DEFS)
# flags_stamp(file, text): every line runs under -n and -q too (the +), so that those see the objects as they are
define flags_stamp
$(1): export R3D_STAMP_TEXT := $(2)
$(1): FORCE
	+@mkdir -p $(OBJDIR); printf '%s\n' "$$$$R3D_STAMP_TEXT" | cmp -s - $$@ || printf '%s\n' "$$$$R3D_STAMP_TEXT" > $$@

endef
ifneq ($(NAME),)
VARIANT := $(LIBDIR)/variant_$(NAME).so
vflags = $(VDEFS) $(DEFS_$(word 1,$(KIND_$(1))))
vstamp = $(OBJDIR)/v$(NAME)_$(1).flags
$(foreach u,$(UNITS) $(ADDONS),$(eval $(call flags_stamp,$(call vstamp,$(u)),$(call unit_cc,$(u),$(call vflags,$(u)))))\
                               $(eval $(call engine_object,v$(NAME),$(u),$(call vflags,$(u)),$(call vstamp,$(u)))))
$(eval $(call engine_library,$(VARIANT),v$(NAME),$(UNITS) $(ADDONS)))
variant: $(VARIANT)
# (when `variant` is a goal, and the run is neither a dry one nor a question: those remove nothing)
ifeq ($(filter variant,$(MAKECMDGOALS))$(findstring n,$(firstword -$(MAKEFLAGS)))$(findstring q,$(firstword -$(MAKEFLAGS))),variant)
$(shell rm -f $(VARIANT))
endif
else
variant:
	$(error make variant NAME=X DEFS="..." [DEFS_CYL= DEFS_TET= DEFS_SPH=]: NAME is not set)
endif
