# Build of the MI355X phonon-transport engine and its host-side pieces.
#
#   make            host model builder + HIP engine + oracle (default)
#   make host       radiative3d_amd/lib/libr3d_host.so   (g++)
#   make engine     radiative3d_amd/lib/libr3d_hip.so    (hipcc, gfx950)
#   make oracle     oracle/libr3d_oracle.so              (g++; test infrastructure)
#   make cli        ./main                               (g++; the reference's command-line surface)
#   make devtest    tests/emul/libr3d_{physics,tables}_device{,_repro}.so  (hipcc, gfx950; test infrastructure)
#
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
HOST_HDR := $(wildcard $(HOSTDIR)/*.hpp) include/r3d.h include/r3d_host.h radiative3d_amd/stats/r3d_window_sums.h
ENGINE_SRC := $(CSRC)/r3d_engine.hip $(CSRC)/r3d_tables_build.hip $(CSRC)/r3d_kernels_kind.hip $(CSRC)/r3d_volume.hip
ENGINE_HDR := $(wildcard $(CSRC)/*.h) include/r3d.h
# The add-ons: what stands beside the engine on its C-ABI, each a directory radiative3d_amd/<name>/ of ONE .hip and
# its headers, which includes $(COMMON)/r3d_entry.h and include/r3d.h and nothing from csrc/.  A new one is a word here.
#   stats  per-bin standard errors from batches (r3d_batch_moments, r3d_run_device_batched), lapse-window sums (r3d_window_sums)
#   views  the two video views of the scatter-event grid (r3d_volume_project, r3d_volume_range_bins)
#   maps   the grid reduced along its frame axis: arrival-time, peak and total maps (r3d_volume_time_maps)
#   arrays the travel-time image of a receiver array with jackknife errors (r3d_array_image, r3d_run_batched_array_image)
ADDONS := stats views maps arrays
addon_src = $(wildcard radiative3d_amd/$(1)/*.hip)
# (arrays/ takes the bin energy and the strand constants from stats/r3d_window_sums.h)
addon_hdr = $(wildcard radiative3d_amd/$(1)/*.h) $(COMMON)/r3d_entry.h include/r3d.h $(if $(filter arrays,$(1)),radiative3d_amd/stats/r3d_window_sums.h)
OBJDIR   := build/obj

# (the default goal is the first target of the file: it has to come before the generated object rules)
.PHONY: default all host engine repro oracle cli devtest clean
default: all
# addon_object(tag, extra flags, add-on): its object in one engine build
define addon_object
$(OBJDIR)/$(1)_$(3).o: $(call addon_src,$(3)) $(call addon_hdr,$(3))
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(2) -c -o $$@ $(call addon_src,$(3))

endef
# engine_objects(tag, extra flags): the objects of one engine build, six of the engine and one per add-on
define engine_objects
$(OBJDIR)/$(1)_engine.o: $(CSRC)/r3d_engine.hip $(ENGINE_HDR)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(2) -c -o $$@ $(CSRC)/r3d_engine.hip
$(OBJDIR)/$(1)_tables.o: $(CSRC)/r3d_tables_build.hip $(ENGINE_HDR)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(2) -c -o $$@ $(CSRC)/r3d_tables_build.hip
$(OBJDIR)/$(1)_volume.o: $(CSRC)/r3d_volume.hip $(ENGINE_HDR) $(COMMON)/r3d_entry.h
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(2) -c -o $$@ $(CSRC)/r3d_volume.hip
$(OBJDIR)/$(1)_cyl.o: $(CSRC)/r3d_kernels_kind.hip $(ENGINE_HDR)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(HIPFLAGS_CYL) $(2) -DR3D_KIND=0 -c -o $$@ $(CSRC)/r3d_kernels_kind.hip
$(OBJDIR)/$(1)_tet.o: $(CSRC)/r3d_kernels_kind.hip $(ENGINE_HDR)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(HIPFLAGS_TET) $(2) -DR3D_KIND=1 -c -o $$@ $(CSRC)/r3d_kernels_kind.hip
$(OBJDIR)/$(1)_sph.o: $(CSRC)/r3d_kernels_kind.hip $(ENGINE_HDR)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(HIPFLAGS_SPH) $(2) -DR3D_KIND=2 -c -o $$@ $(CSRC)/r3d_kernels_kind.hip
$(foreach a,$(ADDONS),$(call addon_object,$(1),$(2),$(a)))
endef
engine_objs = $(foreach a,$(ADDONS),$(OBJDIR)/$(1)_$(a).o) $(OBJDIR)/$(1)_engine.o $(OBJDIR)/$(1)_tables.o $(OBJDIR)/$(1)_volume.o $(OBJDIR)/$(1)_cyl.o $(OBJDIR)/$(1)_tet.o $(OBJDIR)/$(1)_sph.o
$(eval $(call engine_objects,main,))
$(eval $(call engine_objects,repro,-DR3D_REPRODUCIBLE -ffp-contract=off))

all: host engine repro oracle cli devtest

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
main: $(MAIN_SRC) $(HOSTDIR)/scatter_out.hpp $(HOSTDIR)/scatter_plan.hpp $(HOSTDIR)/batch_out.hpp $(HOSTDIR)/batch_plan.hpp \
      $(LIBDIR)/libr3d_host.so $(LIBDIR)/libr3d_hip.so $(ENGINE_HDR)
	$(CXX) $(CXXFLAGS) -pthread -o $@ $(MAIN_SRC) -L$(LIBDIR) -lr3d_host -lr3d_hip \
	    -Wl,-rpath,'$$ORIGIN/$(LIBDIR)' -Wl,-rpath,/opt/rocm/lib

$(LIBDIR)/libr3d_host.so: $(HOST_SRC) $(HOST_HDR)
	@mkdir -p $(LIBDIR)
	$(CXX) $(CXXFLAGS) -shared -pthread -o $@ $(HOST_SRC)

# (librccl is bound at first use, csrc/r3d_rccl.h: the copy already in the process if there is one)
RCCL_LIBS ?= -ldl
$(LIBDIR)/libr3d_hip.so: $(call engine_objs,main)
	@mkdir -p $(LIBDIR)
	$(HIPCC) --offload-arch=gfx950 -shared -pthread -o $@ $(call engine_objs,main) $(RCCL_LIBS)

$(LIBDIR)/libr3d_hip_repro.so: $(call engine_objs,repro)
	@mkdir -p $(LIBDIR)
	$(HIPCC) --offload-arch=gfx950 -shared -pthread -o $@ $(call engine_objs,repro) $(RCCL_LIBS)

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
DEVTEST_SRC := tests/emul/physics_device.hip
DEVTEST_HDR := tests/emul/physics_cases.h $(ENGINE_HDR)
devtest: tests/emul/libr3d_physics_device.so tests/emul/libr3d_physics_device_repro.so \
         tests/emul/libr3d_tables_device.so tests/emul/libr3d_tables_device_repro.so
tests/emul/libr3d_physics_device.so: $(DEVTEST_SRC) $(DEVTEST_HDR) $(OBJDIR)/main_tables.o
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $(OBJDIR)/main_tables.o $(DEVTEST_SRC)
tests/emul/libr3d_physics_device_repro.so: $(DEVTEST_SRC) $(DEVTEST_HDR) $(OBJDIR)/repro_tables.o
	$(HIPCC) $(HIPFLAGS) -DR3D_REPRODUCIBLE -ffp-contract=off -shared -o $@ $(OBJDIR)/repro_tables.o $(DEVTEST_SRC)
# The table builders entry by entry (tests/test_tables_build_device.py): thin test-only entries linked with the table
# OBJECTS of the two engine builds -- the code libr3d_hip.so and libr3d_hip_repro.so carry, not a sibling compilation.
TABTEST_SRC := tests/emul/tables_device.hip
tests/emul/libr3d_tables_device.so: $(TABTEST_SRC) $(ENGINE_HDR) $(OBJDIR)/main_tables.o
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $(OBJDIR)/main_tables.o $(TABTEST_SRC)
tests/emul/libr3d_tables_device_repro.so: $(TABTEST_SRC) $(ENGINE_HDR) $(OBJDIR)/repro_tables.o
	$(HIPCC) $(HIPFLAGS) -DR3D_REPRODUCIBLE -ffp-contract=off -shared -o $@ $(OBJDIR)/repro_tables.o $(TABTEST_SRC)

clean:
	rm -f $(LIBDIR)/*.so oracle/*.so tests/emul/libr3d_physics_device*.so tests/emul/libr3d_tables_device*.so main
	rm -rf $(OBJDIR)

# Developer variants of the engine (timing-only / diagnostic builds, never shipped as libr3d_hip.so;
# the only builds that say -DR3D_DEV_BUILD, without which the R3D_ABLATE_* / R3D_PHASE_TIMING switches
# are a compile error -- csrc/r3d_tables.h):
#   make variant NAME=PHASE DEFS="-DR3D_PHASE_TIMING"   ->  radiative3d_amd/lib/variant_PHASE.so
# run through the tools with R3D_HIP_LIB=radiative3d_amd/lib/variant_PHASE.so (tools/time_chain.py,
# tools/pool_stats.py pass it to Engine(lib=...); the library itself reads no environment).
# Every object is compiled afresh and each compile's status is checked: a failed one cannot leave
# an older object to be linked in its place.
VOBJ = $(OBJDIR)/v$(NAME)
VDEFS = -DR3D_DEV_BUILD $(DEFS)
VOBJS = $(foreach o,engine tables volume cyl tet sph $(ADDONS),$(VOBJ)_$(o).o)
variant:
	@mkdir -p $(OBJDIR)
	rm -f $(VOBJS) $(LIBDIR)/variant_$(NAME).so
	$(HIPCC) $(HIPFLAGS) $(VDEFS) -c -o $(VOBJ)_engine.o $(CSRC)/r3d_engine.hip & p1=$$!; \
	$(HIPCC) $(HIPFLAGS) $(VDEFS) -c -o $(VOBJ)_tables.o $(CSRC)/r3d_tables_build.hip & p2=$$!; \
	$(HIPCC) $(HIPFLAGS) $(VDEFS) -c -o $(VOBJ)_volume.o $(CSRC)/r3d_volume.hip & p6=$$!; \
	$(foreach a,$(ADDONS),$(HIPCC) $(HIPFLAGS) $(VDEFS) -c -o $(VOBJ)_$(a).o $(call addon_src,$(a)) & p_$(a)=$$!;) \
	$(HIPCC) $(HIPFLAGS) $(HIPFLAGS_CYL) $(VDEFS) $(DEFS_CYL) -DR3D_KIND=0 -c -o $(VOBJ)_cyl.o $(CSRC)/r3d_kernels_kind.hip & p3=$$!; \
	$(HIPCC) $(HIPFLAGS) $(HIPFLAGS_TET) $(VDEFS) $(DEFS_TET) -DR3D_KIND=1 -c -o $(VOBJ)_tet.o $(CSRC)/r3d_kernels_kind.hip & p4=$$!; \
	$(HIPCC) $(HIPFLAGS) $(HIPFLAGS_SPH) $(VDEFS) $(DEFS_SPH) -DR3D_KIND=2 -c -o $(VOBJ)_sph.o $(CSRC)/r3d_kernels_kind.hip & p5=$$!; \
	rc=0; for p in $$p1 $$p2 $$p3 $$p4 $$p5 $$p6 $(foreach a,$(ADDONS),$$p_$(a)); do wait $$p || rc=1; done; exit $$rc
	$(HIPCC) --offload-arch=gfx950 -shared -pthread -o $(LIBDIR)/variant_$(NAME).so $(VOBJS) $(RCCL_LIBS)
