# Top-level build: the product (librt_hip.so: HIP kernels + C ABI; librt_host.so: C++ host side) and the
# test oracle (oracle/liboracle.so).  Everything is built IN-TREE so that the .so files travel with gpurun.
#
# The kernels are built for gfx950 only, with contraction OFF: fused multiply-adds appear only where the source
# writes them (arithmetic contract v1); sqrt and division stay correctly rounded (hipcc default).

HIPCC    ?= /opt/rocm/bin/hipcc
CXX      ?= g++
LIBDIR   := rt_amd/lib
HIPFLAGS := --offload-arch=gfx950 -std=c++17 -O3 -fPIC -ffp-contract=off -fno-fast-math -Wall -Wextra -Wno-unused-parameter
HOSTFLAGS:= -std=c++20 -O2 -fPIC -Wall -Wextra

HIPFLAGS += -fvisibility=hidden
# No SLP vectorisation: it pairs the kernels' float arithmetic into v_pk_fma/mul/add_f32, which issue at half rate on this chip
# (two of them cost what four plain instructions do, profiles/r04/valu_issue_costs.txt) and need their operands in even-aligned
# register pairs — moves, and a higher register count.  Measured on the contract-v4 kernels: headline 2.28 -> 2.14 ms,
# basic + plane 2.74 -> 2.62, tilted camera 2.80 -> 2.62 (profiles/r05/codegen_ab.txt).
HIPFLAGS += -fno-slp-vectorize
API_UNITS := context scene frame render frame_call passes multi group denoise temporal adaptive upsample tonemap bloom
HIP_HDR  := rt_amd/csrc/kernels.hpp rt_amd/csrc/launch_plan.hpp rt_amd/csrc/progressive.hpp rt_amd/csrc/denoise.hpp rt_amd/csrc/denoise_rules.hpp rt_amd/csrc/temporal.hpp rt_amd/csrc/reproject_rules.hpp rt_amd/csrc/adaptive.hpp rt_amd/csrc/adaptive_rules.hpp rt_amd/csrc/upsample.hpp rt_amd/csrc/upsample_rules.hpp rt_amd/csrc/tonemap.hpp rt_amd/csrc/tonemap_rules.hpp rt_amd/csrc/bloom.hpp rt_amd/csrc/bloom_rules.hpp rt_amd/csrc/lights.hpp rt_amd/csrc/lens.hpp rt_amd/csrc/lens_rules.hpp rt_amd/csrc/sky_band.hpp rt_amd/csrc/centre_ray.hpp rt_amd/csrc/frame_setup.hpp rt_amd/csrc/contract.hpp rt_amd/csrc/scan.hpp rt_amd/csrc/bvh_scan.hpp rt_amd/csrc/bvh.hpp rt_amd/csrc/box_bvh.hpp rt_amd/csrc/box_bvh_scan.hpp rt_amd/csrc/scan_streamed.hpp rt_amd/csrc/handover.hpp rt_amd/csrc/pixel_output.hpp rt_amd/csrc/lane_state.hpp rt_amd/csrc/queue_build.hpp rt_amd/csrc/camera_forms.hpp rt_amd/csrc/bvh_build.hpp rt_amd/csrc/bvh_build_device.hpp rt_amd/csrc/frame_group.hpp rt_amd/csrc/delivery.hpp rt_amd/csrc/internal.hpp include/rt_hip.h
HOST_SRC := rt_amd/host/host_capi.cpp rt_amd/host/scene.cpp rt_amd/host/toml_subset.cpp
HOST_HDR := $(wildcard rt_amd/host/*.hpp) rt_amd/host/host_capi.h rt_amd/host/named_colours.inc include/rt_hip.h

all: $(LIBDIR)/librt_hip.so $(LIBDIR)/librt_hip_kat.so $(LIBDIR)/librt_host.so rt_amd/bin/rt_headless tests/native/lbvh_reference tests/native/libbox_reference.so tests/native/libdenoise_reference.so tests/native/libreproject_reference.so tests/native/libadaptive_reference.so tests/native/liblight_reference.so tests/native/libdirect_reference.so tests/native/libupsample_reference.so tests/native/libtonemap_reference.so tests/native/libbloom_reference.so tests/native/liblens_reference.so oracle

# kernels.hip is compiled twice: the parity contract (contraction off), and RT_HIP_FLAG_FAST's arithmetic
# (-DRT_HIP_FAST_BUILD -ffp-contract=fast: only launch_render_fast comes out of that one)
FASTFLAGS := $(filter-out -ffp-contract=off,$(HIPFLAGS)) -ffp-contract=fast -DRT_HIP_FAST_BUILD
OBJDIR   := build/obj$(NAME)
HIP_OBJS := $(OBJDIR)/kernels.o $(OBJDIR)/kernels_fast.o $(API_UNITS:%=$(OBJDIR)/%.o) $(OBJDIR)/delivery.o $(OBJDIR)/bvh.o $(OBJDIR)/box_bvh.o $(OBJDIR)/bvh_build.o $(OBJDIR)/launch_plan.o $(OBJDIR)/frame_setup.o $(OBJDIR)/progressive.o $(OBJDIR)/denoise_params.o $(OBJDIR)/temporal_params.o $(OBJDIR)/adaptive_params.o $(OBJDIR)/upsample_params.o $(OBJDIR)/tonemap_params.o $(OBJDIR)/bloom_params.o $(OBJDIR)/lights.o $(OBJDIR)/lens.o $(OBJDIR)/sky_band.o $(OBJDIR)/sky_band_rule.o

$(OBJDIR)/kernels.o: rt_amd/csrc/kernels.hip $(HIP_HDR)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(DEFS) -c $< -o $@
$(OBJDIR)/kernels_fast.o: rt_amd/csrc/kernels.hip $(HIP_HDR)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(FASTFLAGS) $(DEFS) -c $< -o $@
$(OBJDIR)/%.o: rt_amd/csrc/%.hip $(HIP_HDR)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(DEFS) -c $< -o $@
# the pixel carrier is plain C++17 (no HIP): the same source is built into tests/native/pixel_carrier_test on the CPU
$(OBJDIR)/delivery.o: rt_amd/csrc/delivery.cpp rt_amd/csrc/delivery.hpp
	@mkdir -p $(OBJDIR)
	$(CXX) -std=c++17 -O2 -fPIC -fvisibility=hidden -Wall -Wextra -c $< -o $@
# the sphere hierarchy's builder (RT_HIP_FLAG_BVH): plain C++17, linked into the product and into the test-only library
$(OBJDIR)/bvh.o: rt_amd/csrc/bvh.cpp rt_amd/csrc/bvh.hpp
	@mkdir -p $(OBJDIR)
	$(CXX) -std=c++17 -O2 -fPIC -fvisibility=hidden -Wall -Wextra -c $< -o $@
# ... and the box hierarchy's (RT_HIP_FLAG_BOX_BVH): the same on both counts
$(OBJDIR)/box_bvh.o: rt_amd/csrc/box_bvh.cpp rt_amd/csrc/box_bvh.hpp rt_amd/csrc/bvh.hpp
	@mkdir -p $(OBJDIR)
	$(CXX) -std=c++17 -O2 -fPIC -fvisibility=hidden -Wall -Wextra -c $< -o $@

# the launch policy (plan_launch): plain C++17 too, and the same source is built into tests/native/launch_plan_dump on the CPU.
# With $(DEFS): it reads RT_HIP_SAMPLE_CHUNK, RT_HIP_RESIDENT_SCALAR_FROM and RT_HIP_QUEUE_KNOBS, which a variant build must see in both compilers
$(OBJDIR)/launch_plan.o: rt_amd/csrc/launch_plan.cpp rt_amd/csrc/launch_plan.hpp include/rt_hip.h
	@mkdir -p $(OBJDIR)
	$(CXX) -std=c++17 -O2 -fPIC -fvisibility=hidden -Wall -Wextra $(DEFS) -c $< -o $@

# the sequencing of a progressive frame's passes (next_pass): plain C++17 too, and the same source is built into tests/native/pass_plan_dump on the CPU
$(OBJDIR)/progressive.o: rt_amd/csrc/progressive.cpp rt_amd/csrc/progressive.hpp rt_amd/csrc/launch_plan.hpp include/rt_hip.h
	@mkdir -p $(OBJDIR)
	$(CXX) -std=c++17 -O2 -fPIC -fvisibility=hidden -Wall -Wextra $(DEFS) -c $< -o $@

# the denoiser's parameters (default_denoise_params, check_denoise_params): plain C++17 too, and the same source is built into
# tests/native/libdenoise_reference.so on the CPU
$(OBJDIR)/denoise_params.o: rt_amd/csrc/denoise.cpp rt_amd/csrc/denoise.hpp include/rt_hip.h
	@mkdir -p $(OBJDIR)
	$(CXX) -std=c++17 -O2 -fPIC -fvisibility=hidden -Wall -Wextra $(DEFS) -c $< -o $@

# temporal accumulation's host-only rules (parameters, forward_view_projection, same_history): plain C++17 too, and the same source is
# built into tests/native/libreproject_reference.so on the CPU
$(OBJDIR)/temporal_params.o: rt_amd/csrc/temporal.cpp rt_amd/csrc/temporal.hpp rt_amd/csrc/progressive.hpp include/rt_hip.h
	@mkdir -p $(OBJDIR)
	$(CXX) -std=c++17 -O2 -fPIC -fvisibility=hidden -Wall -Wextra $(DEFS) -c $< -o $@

# adaptive sampling's host-only rules (parameters, the sequencing of an accumulation): plain C++17 too, and the same source is built
# into tests/native/libadaptive_reference.so and tests/native/adaptive_plan_dump on the CPU
$(OBJDIR)/adaptive_params.o: rt_amd/csrc/adaptive.cpp rt_amd/csrc/adaptive.hpp rt_amd/csrc/progressive.hpp rt_amd/csrc/launch_plan.hpp include/rt_hip.h
	@mkdir -p $(OBJDIR)
	$(CXX) -std=c++17 -O2 -fPIC -fvisibility=hidden -Wall -Wextra $(DEFS) -c $< -o $@

# guided upsampling's host-only rules (parameters, size checks, the low-size rule): plain C++17 too, and the same source is built into
# tests/native/libupsample_reference.so and the program of `make sanitize-upsample` on the CPU
$(OBJDIR)/upsample_params.o: rt_amd/csrc/upsample.cpp rt_amd/csrc/upsample.hpp include/rt_hip.h
	@mkdir -p $(OBJDIR)
	$(CXX) -std=c++17 -O2 -fPIC -fvisibility=hidden -Wall -Wextra $(DEFS) -c $< -o $@

# tone mapping's host-only rules (parameters, the CURVE[:EXPOSURE] parser): plain C++17 too, and the same source is built into
# tests/native/libtonemap_reference.so and the program of `make sanitize-tonemap` on the CPU
$(OBJDIR)/tonemap_params.o: rt_amd/csrc/tonemap.cpp rt_amd/csrc/tonemap.hpp include/rt_hip.h
	@mkdir -p $(OBJDIR)
	$(CXX) -std=c++17 -O2 -fPIC -fvisibility=hidden -Wall -Wextra $(DEFS) -c $< -o $@

# bloom's host-only rules (parameters, the level plan, the key=value parser): plain C++17 too, and the same source is built into
# tests/native/libbloom_reference.so and the program of `make sanitize-bloom` on the CPU.  Contraction off, spelled out: norm and gain
# are defined by their order of operations
$(OBJDIR)/bloom_params.o: rt_amd/csrc/bloom.cpp rt_amd/csrc/bloom.hpp rt_amd/csrc/bloom_rules.hpp include/rt_hip.h
	@mkdir -p $(OBJDIR)
	$(CXX) -std=c++17 -O2 -fPIC -fvisibility=hidden -ffp-contract=off -Wall -Wextra $(DEFS) -c $< -o $@

# emissive materials' host-only rules (the emission table's checks, rt_hip_lights_from_spec): plain C++17 too, and the same source is
# built into tests/native/light_plan_dump and the program of `make sanitize-lights` on the CPU
$(OBJDIR)/lights.o: rt_amd/csrc/lights.cpp rt_amd/csrc/lights.hpp include/rt_hip.h
	@mkdir -p $(OBJDIR)
	$(CXX) -std=c++17 -O2 -fPIC -fvisibility=hidden -Wall -Wextra $(DEFS) -c $< -o $@

# the thin lens' host-only rules (the lens' checks, rt_hip_lens_from_spec, the ten lens words of a frame): plain C++17 too, and the same source
# is built into tests/native/liblens_reference.so, tests/native/lens_plan_dump and the program of `make sanitize-lens` on the CPU.
# Contraction off, spelled out: the binary64 constants are defined by their order of operations
$(OBJDIR)/lens.o: rt_amd/csrc/lens.cpp rt_amd/csrc/lens.hpp rt_amd/csrc/frame_setup.hpp rt_amd/csrc/launch_plan.hpp include/rt_hip.h
	@mkdir -p $(OBJDIR)
	$(CXX) -std=c++17 -O2 -fPIC -fvisibility=hidden -ffp-contract=off -Wall -Wextra $(DEFS) -c $< -o $@

# the sky band's rule (sky_band_rows: how many rows from the top of a frame provably see nothing): plain C++17 too, and the same
# source is built into tests/native/sky_band_dump and the program of `make sanitize-sky-band` on the CPU.  (sky_band.o is the band's kernel,
# sky_band.hip, by the pattern rule above.)
$(OBJDIR)/sky_band_rule.o: rt_amd/csrc/sky_band.cpp rt_amd/csrc/sky_band.hpp rt_amd/csrc/frame_setup.hpp rt_amd/csrc/launch_plan.hpp include/rt_hip.h
	@mkdir -p $(OBJDIR)
	$(CXX) -std=c++17 -O2 -fPIC -fvisibility=hidden -Wall -Wextra $(DEFS) -c $< -o $@

# the refusals of a render request and the kernels' per-frame constants (check_render_request, make_frame_params): plain C++17, and the
# same source is built into tests/native/frame_setup_dump on the CPU.  Contraction off, spelled out: the camera's binary64 constants are
# defined by their order of operations
$(OBJDIR)/frame_setup.o: rt_amd/csrc/frame_setup.cpp rt_amd/csrc/frame_setup.hpp rt_amd/csrc/launch_plan.hpp include/rt_hip.h
	@mkdir -p $(OBJDIR)
	$(CXX) -std=c++17 -O2 -fPIC -fvisibility=hidden -ffp-contract=off -Wall -Wextra $(DEFS) -c $< -o $@

# the product: exports the C entry points of include/rt_hip.h and nothing else
$(LIBDIR)/librt_hip.so: $(HIP_OBJS)
	@mkdir -p $(LIBDIR)
	$(HIPCC) --offload-arch=gfx950 -fPIC -shared -o $@ $(HIP_OBJS) -L/opt/rocm/lib -lrccl -lpthread
	python3 tools/kernel_sources_hash.py > $(LIBDIR)/librt_hip.kernels.sha16   # what THIS binary's kernels were compiled from (bench.py, profiles)

# test-only: the known-answer entry points of include/rt_hip_kat.h (never shipped; loads next to librt_hip.so)
# (with its own copies of both builders of the sphere hierarchy: librt_hip.so exports neither)
# (kat_fast.o: contract.hpp's fast leaf functions as RT_HIP_FLAG_FAST's build of the kernels compiles them, for rt_hip_kat_fast_math — FASTFLAGS,
# this library only: nothing of it is linked into librt_hip.so)
$(LIBDIR)/librt_hip_kat.so: $(OBJDIR)/kat.o $(OBJDIR)/kat_fast.o $(OBJDIR)/bvh.o $(OBJDIR)/box_bvh.o $(OBJDIR)/bvh_build.o $(LIBDIR)/librt_hip.so
	$(HIPCC) --offload-arch=gfx950 -fPIC -shared -o $@ $(OBJDIR)/kat.o $(OBJDIR)/kat_fast.o $(OBJDIR)/bvh.o $(OBJDIR)/box_bvh.o $(OBJDIR)/bvh_build.o -L$(LIBDIR) -lrt_hip -Wl,-rpath,'$$ORIGIN' -L/opt/rocm/lib -lrccl
$(OBJDIR)/kat.o: include/rt_hip_kat.h
$(OBJDIR)/kat_fast.o: rt_amd/csrc/kat_fast.hip rt_amd/csrc/contract.hpp rt_amd/csrc/frame_setup.hpp
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(FASTFLAGS) $(DEFS) -c $< -o $@

$(LIBDIR)/librt_host.so: $(HOST_SRC) $(HOST_HDR)
	@mkdir -p $(LIBDIR)
	$(CXX) $(HOSTFLAGS) -shared -o $@ $(HOST_SRC)

# experiment builds for tools/gpu_ab.py: make variant NAME=x DEFS="-DRT_HIP_SOMETHING=1" -> rt_amd/lib/librt_hip_x.so
# (objects under build/obj<NAME>; an experiment library carries the known-answer and debug entry points itself)
variant: $(HIP_OBJS) $(OBJDIR)/kat.o $(OBJDIR)/kat_fast.o
	@mkdir -p $(LIBDIR)
	$(HIPCC) --offload-arch=gfx950 -fPIC -shared -o $(LIBDIR)/librt_hip_$(NAME).so $(HIP_OBJS) $(OBJDIR)/kat.o $(OBJDIR)/kat_fast.o -L/opt/rocm/lib -lrccl -lpthread

# windowless driver: the registry, the hip_ray_tracer plug-in and the scene loader, linked against the C ABI only
# (the plug-in's body is shim/rt_hip_plugin.hpp, which finds <rt_hip.h> on the include path as it does inside rt: -Iinclude)
HEADLESS_SRC := rt_amd/host/main.cpp rt_amd/host/hip_ray_tracer.cpp rt_amd/host/scene.cpp rt_amd/host/toml_subset.cpp
rt_amd/bin/rt_headless: $(HEADLESS_SRC) $(HOST_HDR) shim/rt_hip_plugin.hpp $(LIBDIR)/librt_hip.so
	@mkdir -p rt_amd/bin
	$(CXX) $(HOSTFLAGS) -Iinclude -o $@ $(HEADLESS_SRC) -L$(LIBDIR) -lrt_hip -Wl,-rpath,'$$ORIGIN/../lib'

# `make sanitize-plugin`: the plug-in behind the main() of tests/native/plugin_calls.cpp — a recording fake of the C entry points it links,
# no GPU — under AddressSanitizer and UndefinedBehaviorSanitizer, run over the RT_HIP_GROUP, RT_HIP_DEVICES and RT_HIP_LIGHTS rows of
# tests/test_plugin_calls.py's matrix (the parsers with buffers of their own, the emission table's upkeep) and held to
# tests/golden/plugin_calls.txt.  CPU only, nothing is loaded into python (it starts the program, one process per row); the binary
# goes to build/ and is run at once
PLUGIN_CALLS_SRC := tests/native/plugin_calls.cpp rt_amd/host/hip_ray_tracer.cpp rt_amd/host/scene.cpp rt_amd/host/toml_subset.cpp
sanitize-plugin: $(PLUGIN_CALLS_SRC) $(HOST_HDR) shim/rt_hip_plugin.hpp
	@mkdir -p build
	$(CXX) -O1 -g -std=c++20 -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -Iinclude -Irt_amd/host $(PLUGIN_CALLS_SRC) -o build/plugin_calls_sanitize
	python3 -m tests.test_plugin_calls check build/plugin_calls_sanitize RT_HIP_GROUP RT_HIP_DEVICES RT_HIP_LIGHTS

# the device builder of the sphere hierarchy restated serially over its own per-element header, g++ alone (tests/test_bvh_lbvh_reference.py
# builds its own copy; this one is for the command line)
tests/native/lbvh_reference: tests/native/lbvh_reference.cpp rt_amd/csrc/bvh_build.hpp
	$(CXX) -std=c++20 -O2 -ffp-contract=off -Wall -Wextra $< -o $@

# the CPU restatement of RT_HIP_FLAG_TRACE_BOXES: the oracle's own translation unit with a test_boxes that hits (it includes
# oracle/cpu_ref.cpp and restates nothing of it), g++ alone, the oracle's strict flags; tests/box_reference.py binds it
tests/native/libbox_reference.so: tests/native/box_reference.cpp oracle/cpu_ref.cpp oracle/cpu_ref.h include/rt_hip.h
	$(CXX) -O2 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fno-math-errno -mfma -Wall -Wextra -shared $< -o $@ -lpthread

# the CPU restatement of the denoiser: the serial filter over rt_amd/csrc/denoise_rules.hpp — the kernels' own text —
# with the oracle's leaf functions (it includes oracle/cpu_ref.cpp), and denoise.cpp as it is; g++ alone, the oracle's strict flags;
# tests/denoise_reference.py binds it
tests/native/libdenoise_reference.so: tests/native/denoise_reference.cpp rt_amd/csrc/denoise_rules.hpp rt_amd/csrc/denoise.cpp rt_amd/csrc/denoise.hpp oracle/cpu_ref.cpp oracle/cpu_ref.h include/rt_hip.h
	$(CXX) -O2 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fno-math-errno -mfma -Wall -Wextra -shared $< rt_amd/csrc/denoise.cpp -o $@ -lpthread

# the CPU restatement of temporal accumulation: the serial loop over rt_amd/csrc/reproject_rules.hpp — the kernel's own
# text — with the oracle's leaf functions and oracle_primary_ray (it includes oracle/cpu_ref.cpp), and temporal.cpp as it is; g++ alone,
# the oracle's strict flags; tests/reproject_reference.py binds it
REPROJECT_REF_SRC := tests/native/reproject_reference.cpp rt_amd/csrc/reproject_rules.hpp rt_amd/csrc/temporal.cpp rt_amd/csrc/temporal.hpp rt_amd/csrc/progressive.hpp oracle/cpu_ref.cpp oracle/cpu_ref.h include/rt_hip.h
tests/native/libreproject_reference.so: $(REPROJECT_REF_SRC)
	$(CXX) -O2 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fno-math-errno -mfma -Wall -Wextra -shared $< rt_amd/csrc/temporal.cpp -o $@ -lpthread

# `make sanitize-temporal`: the same two sources behind a main() of their own (a 70 x 41 frame whose projections leave the frame, a
# singular matrix, every parameter refusal) under AddressSanitizer and UndefinedBehaviorSanitizer.  CPU only, nothing is loaded into
# python; the binary goes to build/ and is run at once
sanitize-temporal: tests/native/reproject_sanitize.cpp $(REPROJECT_REF_SRC)
	@mkdir -p build
	$(CXX) -O1 -g -std=c++17 -ffp-contract=off -fno-fast-math -fno-math-errno -mfma -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer $< rt_amd/csrc/temporal.cpp -o build/reproject_sanitize -lpthread
	build/reproject_sanitize

# `make sanitize-box-bvh`: the box hierarchy's host builder behind a main() of its own — the counts, the identical boxes, the depth-24
# chain, lo > hi, NaN and infinite corners of tests/test_box_bvh_build.py, each tree checked for coverage, exact unions and depth —
# under AddressSanitizer and UndefinedBehaviorSanitizer.  CPU only, nothing is loaded into python; the binary goes to build/ and is
# run at once
sanitize-box-bvh: tests/native/box_bvh_sanitize.cpp rt_amd/csrc/box_bvh.cpp rt_amd/csrc/box_bvh.hpp rt_amd/csrc/bvh.hpp
	@mkdir -p build
	$(CXX) -O1 -g -std=c++17 -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer $< rt_amd/csrc/box_bvh.cpp -o build/box_bvh_sanitize
	build/box_bvh_sanitize

# the CPU restatement of adaptive sampling's update step: the serial loop over rt_amd/csrc/adaptive_rules.hpp — the
# kernel's own text — finishing every pixel with the oracle's pack (it includes oracle/cpu_ref.cpp), and adaptive.cpp and progressive.cpp
# as they are; g++ alone, the oracle's strict flags; tests/adaptive_reference.py binds it
ADAPTIVE_REF_SRC := tests/native/adaptive_reference.cpp rt_amd/csrc/adaptive_rules.hpp rt_amd/csrc/adaptive.cpp rt_amd/csrc/adaptive.hpp rt_amd/csrc/progressive.cpp rt_amd/csrc/progressive.hpp rt_amd/csrc/launch_plan.hpp oracle/cpu_ref.cpp oracle/cpu_ref.h include/rt_hip.h
tests/native/libadaptive_reference.so: $(ADAPTIVE_REF_SRC)
	$(CXX) -O2 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fno-math-errno -mfma -Wall -Wextra -shared $< rt_amd/csrc/adaptive.cpp rt_amd/csrc/progressive.cpp -o $@ -lpthread

# `make sanitize-adaptive`: the host-only unit and the serial restatement behind a main() of their own (every parameter refusal, an
# accumulation sequenced to completion by the cap and by "no pixel active", update steps over a 37 x 23 frame with stopped pixels, NaN
# sums and a short last pass) under AddressSanitizer and UndefinedBehaviorSanitizer.  CPU only, nothing is loaded into python; the
# binary goes to build/ and is run at once
sanitize-adaptive: tests/native/adaptive_sanitize.cpp $(ADAPTIVE_REF_SRC)
	@mkdir -p build
	$(CXX) -O1 -g -std=c++17 -ffp-contract=off -fno-fast-math -fno-math-errno -mfma -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer $< tests/native/adaptive_reference.cpp rt_amd/csrc/adaptive.cpp rt_amd/csrc/progressive.cpp -o build/adaptive_sanitize -lpthread
	build/adaptive_sanitize

# the CPU restatement of RT_HIP_FLAG_EMISSION: the oracle's own translation unit with a trace loop that knows lights (it
# includes oracle/cpu_ref.cpp and restates nothing else of it), g++ alone, the oracle's strict flags; tests/light_reference.py binds it
tests/native/liblight_reference.so: tests/native/light_reference.cpp oracle/cpu_ref.cpp oracle/cpu_ref.h include/rt_hip.h
	$(CXX) -O2 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fno-math-errno -mfma -Wall -Wextra -shared $< -o $@ -lpthread

# `make sanitize-lights`: rt_hip_lights_from_spec and the emission table's checks behind a main() of their own — every well-formed and
# malformed shape of tests/test_light_spec.py, truncated and oversized specs — under AddressSanitizer and UndefinedBehaviorSanitizer.
# CPU only, nothing is loaded into python; the binary goes to build/ and is run at once
sanitize-lights: tests/native/light_spec_sanitize.cpp rt_amd/csrc/lights.cpp rt_amd/csrc/lights.hpp include/rt_hip.h
	@mkdir -p build
	$(CXX) -O1 -g -std=c++17 -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer $< rt_amd/csrc/lights.cpp -o build/light_spec_sanitize
	build/light_spec_sanitize

# `make sanitize-sky-band`: the sky band's rule behind the main() of tests/native/sky_band_dump.cpp, fed the constructed cases of
# tests/test_sky_band_rule.py from tests/golden/sky_band_cases.txt (written by `python -m tests.test_sky_band_rule`, held to it by that file's tests), under AddressSanitizer and UndefinedBehaviorSanitizer.  CPU only, nothing is
# loaded into python; the binary goes to build/ and is run at once
sanitize-sky-band: tests/native/sky_band_dump.cpp rt_amd/csrc/sky_band.cpp rt_amd/csrc/sky_band.hpp rt_amd/csrc/frame_setup.cpp rt_amd/csrc/frame_setup.hpp
	@mkdir -p build
	$(CXX) -O1 -g -std=c++17 -ffp-contract=off -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer $< rt_amd/csrc/sky_band.cpp rt_amd/csrc/frame_setup.cpp -o build/sky_band_sanitize
	build/sky_band_sanitize < tests/golden/sky_band_cases.txt > /dev/null

# the CPU restatement of RT_HIP_FLAG_DIRECT_LIGHT: light_reference.cpp's way — the oracle's own translation unit, only the
# trace loop restated — with the vertex rule of rt_amd/csrc/direct_light_rules.hpp, the text the device runs; tests/direct_reference.py binds it
tests/native/libdirect_reference.so: tests/native/direct_reference.cpp rt_amd/csrc/direct_light_rules.hpp oracle/cpu_ref.cpp oracle/cpu_ref.h include/rt_hip.h
	$(CXX) -O2 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fno-math-errno -mfma -Wall -Wextra -shared $< -o $@ -lpthread

# the CPU restatement of guided upsampling: the serial loop over rt_amd/csrc/upsample_rules.hpp — the kernel's own text —
# with the oracle's leaf functions (it includes oracle/cpu_ref.cpp), and upsample.cpp as it is; g++ alone, the oracle's strict flags;
# tests/upsample_reference.py binds it
UPSAMPLE_REF_SRC := tests/native/upsample_reference.cpp rt_amd/csrc/upsample_rules.hpp rt_amd/csrc/denoise_rules.hpp rt_amd/csrc/upsample.cpp rt_amd/csrc/upsample.hpp oracle/cpu_ref.cpp oracle/cpu_ref.h include/rt_hip.h
tests/native/libupsample_reference.so: $(UPSAMPLE_REF_SRC)
	$(CXX) -O2 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fno-math-errno -mfma -Wall -Wextra -shared $< rt_amd/csrc/upsample.cpp -o $@ -lpthread

# `make sanitize-upsample`: the host-only unit and the serial restatement behind a main() of their own (ragged sizes — 1 x 1, 37 x 3 from
# 1 x 1, 70 x 41 from 18 x 11, w == W — with NaN and infinite taps, every parameter, size and factor refusal) under AddressSanitizer and
# UndefinedBehaviorSanitizer.  CPU only, nothing is loaded into python; the binary goes to build/ and is run at once
sanitize-upsample: tests/native/upsample_sanitize.cpp $(UPSAMPLE_REF_SRC)
	@mkdir -p build
	$(CXX) -O1 -g -std=c++17 -ffp-contract=off -fno-fast-math -fno-math-errno -mfma -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer $< tests/native/upsample_reference.cpp rt_amd/csrc/upsample.cpp -o build/upsample_sanitize -lpthread
	build/upsample_sanitize

# the CPU restatement of tone mapping: the serial loops over rt_amd/csrc/tonemap_rules.hpp — the kernels' own text —
# finishing every pixel with the oracle's square root and pack (it includes oracle/cpu_ref.cpp), and tonemap.cpp as it is; g++ alone,
# the oracle's strict flags; tests/tonemap_reference.py binds it
TONEMAP_REF_SRC := tests/native/tonemap_reference.cpp rt_amd/csrc/tonemap_rules.hpp rt_amd/csrc/tonemap.cpp rt_amd/csrc/tonemap.hpp oracle/cpu_ref.cpp oracle/cpu_ref.h include/rt_hip.h
tests/native/libtonemap_reference.so: $(TONEMAP_REF_SRC)
	$(CXX) -O2 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fno-math-errno -mfma -Wall -Wextra -shared $< rt_amd/csrc/tonemap.cpp -o $@ -lpthread

# `make sanitize-tonemap`: the host-only unit and the serial restatement behind a main() of their own (ragged sizes from 1 x 1, frames of
# NaN, infinities, negatives and zeros, every bin, every rank cut, the adaptation sequence, every parameter refusal, the parser on
# well-formed, malformed, truncated and oversized texts) under AddressSanitizer and UndefinedBehaviorSanitizer.  CPU only, nothing is
# loaded into python; the binary goes to build/ and is run at once
sanitize-tonemap: tests/native/tonemap_sanitize.cpp $(TONEMAP_REF_SRC)
	@mkdir -p build
	$(CXX) -O1 -g -std=c++17 -ffp-contract=off -fno-fast-math -fno-math-errno -mfma -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer $< tests/native/tonemap_reference.cpp rt_amd/csrc/tonemap.cpp -o build/tonemap_sanitize -lpthread
	build/tonemap_sanitize

# the CPU restatement of bloom: the serial loops over rt_amd/csrc/bloom_rules.hpp — the kernels' own text — and
# bloom.cpp as it is; g++ alone, the oracle's strict flags; tests/bloom_reference.py binds it
BLOOM_REF_SRC := tests/native/bloom_reference.cpp rt_amd/csrc/bloom_rules.hpp rt_amd/csrc/bloom.cpp rt_amd/csrc/bloom.hpp include/rt_hip.h
tests/native/libbloom_reference.so: $(BLOOM_REF_SRC)
	$(CXX) -O2 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fno-math-errno -mfma -Wall -Wextra -shared $< rt_amd/csrc/bloom.cpp -o $@

# `make sanitize-bloom`: the host-only unit and the serial restatement behind a main() of their own (ragged sizes from 1 x 1, frames of
# NaN, infinities, negatives and denormals, every level count, in place, every parameter refusal, the parser on well-formed, malformed,
# truncated and oversized texts) under AddressSanitizer and UndefinedBehaviorSanitizer.  CPU only, nothing is loaded into python; the
# binary goes to build/ and is run at once
sanitize-bloom: tests/native/bloom_sanitize.cpp $(BLOOM_REF_SRC)
	@mkdir -p build
	$(CXX) -O1 -g -std=c++17 -ffp-contract=off -fno-fast-math -fno-math-errno -mfma -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer $< tests/native/bloom_reference.cpp rt_amd/csrc/bloom.cpp -o build/bloom_sanitize
	build/bloom_sanitize

# the CPU restatement of RT_HIP_FLAG_THIN_LENS: light_reference.cpp's way — the oracle's own translation unit, only
# render_pixel's sample loop restated — with the rules of rt_amd/csrc/lens_rules.hpp, the text the device runs, and lens.cpp and
# frame_setup.cpp as they are; g++ alone, the oracle's strict flags; tests/lens_reference.py binds it
LENS_REF_SRC := tests/native/lens_reference.cpp rt_amd/csrc/lens_rules.hpp rt_amd/csrc/lens.cpp rt_amd/csrc/lens.hpp rt_amd/csrc/frame_setup.cpp rt_amd/csrc/frame_setup.hpp rt_amd/csrc/launch_plan.hpp oracle/cpu_ref.cpp oracle/cpu_ref.h include/rt_hip.h
tests/native/liblens_reference.so: $(LENS_REF_SRC)
	$(CXX) -O2 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fno-math-errno -mfma -Wall -Wextra -shared $< rt_amd/csrc/lens.cpp rt_amd/csrc/frame_setup.cpp -o $@ -lpthread

# `make sanitize-lens`: the parser, the lens' checks and the lens words behind a main() of their own — every well-formed and malformed text
# of tests/test_lens_host.py, truncated and oversized specs, every refused value, the words of an axis-aligned, a tilted and a 1-pixel
# frame and of a matrix without an eye — under AddressSanitizer and UndefinedBehaviorSanitizer.  CPU only, nothing is loaded into python;
# the binary goes to build/ and is run at once
sanitize-lens: tests/native/lens_sanitize.cpp rt_amd/csrc/lens.cpp rt_amd/csrc/lens.hpp rt_amd/csrc/frame_setup.cpp rt_amd/csrc/frame_setup.hpp include/rt_hip.h
	@mkdir -p build
	$(CXX) -O1 -g -std=c++17 -ffp-contract=off -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer $< rt_amd/csrc/lens.cpp rt_amd/csrc/frame_setup.cpp -o build/lens_sanitize
	build/lens_sanitize

oracle:
	$(MAKE) -C oracle

# tests/native/soagen_columns.cpp against the reference's own vendored container runtime, compiled from where it lies under
# /root/reference (nothing is copied; the reference tree exists in the build container only).  The binary goes to oracle/_ref/:
# git-ignored, not gpurun-ignored — the GPU box runs it with --gpu (tests/test_soagen_columns.py).
SOAGEN_DIR := /root/reference/vendor
ifneq ($(wildcard $(SOAGEN_DIR)/soagen.hpp),)
all: oracle/_ref/soagen_columns
oracle/_ref/soagen_columns: tests/native/soagen_columns.cpp $(LIBDIR)/librt_hip.so oracle include/rt_hip.h oracle/cpu_ref.h
	@mkdir -p oracle/_ref
	$(CXX) -std=c++20 -O1 -Wall -Wextra -I$(SOAGEN_DIR) -Iinclude -Ioracle $< -o $@ -L$(LIBDIR) -lrt_hip -Loracle -loracle -Wl,-rpath,'$$ORIGIN/../../$(LIBDIR)' -Wl,-rpath,'$$ORIGIN/..'
endif

clean:
	rm -f $(LIBDIR)/*.so rt_amd/bin/rt_headless tests/native/lbvh_reference tests/native/libbox_reference.so tests/native/libdenoise_reference.so tests/native/libreproject_reference.so tests/native/libadaptive_reference.so tests/native/liblight_reference.so tests/native/libdirect_reference.so tests/native/libupsample_reference.so tests/native/libtonemap_reference.so tests/native/libbloom_reference.so tests/native/liblens_reference.so
	$(MAKE) -C oracle clean

.PHONY: all oracle clean variant sanitize-temporal sanitize-box-bvh sanitize-adaptive sanitize-lights sanitize-sky-band sanitize-upsample sanitize-tonemap sanitize-bloom sanitize-plugin sanitize-lens
