# Builds libmimo_hip.so (gfx950).  `python -c "import __graft_entry__ as g; g.build()"` calls this.  (The oracle is pure
# Python on torch's CPU operators and the reference has no native sources: nothing else to compile.)
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
CSRC := mimo_unet_amd/csrc
SRCS := $(CSRC)/conv3x3.hip $(CSRC)/conv_thin.hip $(CSRC)/conv_bf16x3.hip $(CSRC)/conv_wide.hip $(CSRC)/wgrad_split.hip $(CSRC)/ew_reduce.hip $(CSRC)/ew_layout.hip $(CSRC)/ew_bn_fwd.hip $(CSRC)/ew_resample.hip $(CSRC)/ew_dropout.hip $(CSRC)/ew_bn_bwd.hip $(CSRC)/ew_head_loss.hip $(CSRC)/perm_draw.hip $(CSRC)/fgsm.hip $(CSRC)/pgd.hip $(CSRC)/monitor.hip $(CSRC)/evidential_eval.hip $(CSRC)/optim.hip $(CSRC)/plan.hip $(CSRC)/ops_api.hip $(CSRC)/eval/eval_stats.hip $(CSRC)/eval/score_rules.hip $(CSRC)/eval/score_evidential.hip $(CSRC)/optim_clip/grad_clip.hip $(CSRC)/data/dataset_gather.hip $(CSRC)/scene/scene_tiles.hip
OBJS := $(SRCS:.hip=.o)
LIB := mimo_unet_amd/libmimo_hip.so
HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -fvisibility=hidden -Wall -Wno-unused-function

# test-only twin of the library: plan.hip compiled together with tests/host/plan_probe.hip, which copies a layer's input and
# pre-activation tensor out of a plan (tests/test_plan_entry_gpu.py) and tells which weight-gradient launch the recipe makes
# (tests/test_wgrad_splits_gpu.py); same objects otherwise, same version script
PROBE := mimo_unet_amd/libmimo_plan_probe.so

all: $(LIB) $(PROBE)

# every compile leaves hipcc's per-kernel resource remarks next to the object (csrc/*.res): scripts/check_resources.py
# fails the build when a kernel that counts its vector-memory operations by hand (LDS-DMA) touches scratch
$(CSRC)/%.o: $(CSRC)/%.hip $(CSRC)/common.h $(CSRC)/pack_layout.h $(CSRC)/conv_recipe.h $(CSRC)/conv_launch.h $(CSRC)/tile_sched.h $(CSRC)/dz_ring.h $(CSRC)/graph_replay.h $(CSRC)/elementwise.h $(CSRC)/ew_device.h $(CSRC)/adam_update.h $(CSRC)/block_reduce.h $(CSRC)/evidential.h $(CSRC)/philox.h $(CSRC)/eval/score_common.h $(CSRC)/eval/student_t.h include/mimo_hip.h
	$(HIPCC) $(HIPFLAGS) -Rpass-analysis=kernel-resource-usage -c $< -o $@ 2> $(@:.o=.res) || (grep -v "remark:" $(@:.o=.res) >&2; false)
	@grep -E "warning:|error:" -A3 $(@:.o=.res) >&2 || true

$(LIB): $(OBJS) $(CSRC)/exports.map
	python3 scripts/check_resources.py $(OBJS:.o=.res)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -Wl,--version-script=$(CSRC)/exports.map -o $@ $(OBJS)

$(CSRC)/plan_probe.o: tests/host/plan_probe.hip $(CSRC)/plan.o
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(PROBE): $(CSRC)/plan_probe.o $(OBJS) $(CSRC)/exports.map
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -Wl,--version-script=$(CSRC)/exports.map -o $@ $(CSRC)/plan_probe.o $(filter-out $(CSRC)/plan.o,$(OBJS))

clean:
	rm -f $(OBJS) $(OBJS:.o=.res) $(LIB) $(PROBE) $(CSRC)/plan_probe.o

.PHONY: all clean
