// mimo_plan: the MIMO U-Net network executor behind the C ABI.  Owns packed weights, saved
// activations, BatchNorm statistics and scratch; sequences the HIP kernels of conv3x3.hip /
// the ew_*.hip operator files for forward, loss and backward on the caller's stream.
//
// Topology restated from the reference (relative to /root/reference):
//   MimoUNet.forward ........... mimo/models/mimo_components/model.py:94-117
//   SubnetworkEncoder .......... model.py:119-175   (S private DoubleConv + Down)
//   SubnetworkCore ............. model.py:178-243   (down2..4, up1..3 on the channel concat)
//   SubnetworkDecoder .......... model.py:246-297   (S private Up + OutConv, stacked)
//   DoubleConv / Down / Up ..... mimo/models/mimo_components/components.py:8-120
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "dz_ring.h"
#include "elementwise.h"
#include "graph_replay.h"

namespace mimo {

static thread_local char g_error[512] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_error, sizeof(g_error), fmt, ap);
  va_end(ap);
}
const char* last_error() { return g_error; }

namespace {

struct TensorInfo {
  std::string name;
  int ndim;
  int64_t shape[4];
  int kind;  // 0 parameter, 1 BN buffer
  int64_t offset;
};

// An activation tensor as seen by consumers: pointer (possibly a channel slice of a wider
// concat buffer), pixel pitch, padded channel count, gradient buffer, and the map from padded
// channel index to the logical channel index inside this tensor (-1 = zero padding).
struct Act {
  float* a = nullptr;
  int ld = 0;
  float* da = nullptr;
  int ldda = 0;
  int Cp = 0, C = 0;
  int N = 0, H = 0, W = 0;
  std::vector<int> chmap;
  int grad_writes = 0;  // run-time counter: first writer assigns, later writers accumulate
  // skip-connection gradient of this tensor, left in the consuming Up block's own padded-domain buffer (channels
  // [0, Cp), pixel pitch skipgrad_ld) until the MaxPool backward of the same tensor folds it in
  const float* skipgrad = nullptr;
  int skipgrad_ld = 0;
  // Pooled gradient of this tensor left in the pooling Down block's own padded-domain buffer (pixel pitch poolgrad_ld) for
  // the BatchNorm backward of the producing convolution(s) to route through the max-pool windows themselves (GS_POOL,
  // elementwise.h): pool_bwd is not launched and `da` is not written.  A channel slice of a concat tensor (down1[s] inside
  // x2cat) finds both gradients on `parent`, at channel offset parent_choff.
  const float* poolgrad = nullptr;
  int poolgrad_ld = 0;
  Act* parent = nullptr;
  int parent_choff = 0;
  // != nullptr: in a TRAINING forward `a` is not written — its readers (the bilinear up-sampling into the next block's
  // concat buffer, the 1x1 head and its backward) take the producing convolution's pre-activation tensor z (pixel pitch
  // z_ld) and apply scale / shift + ReLU themselves (round 4; Up blocks without dropout in split16)
  const float *z = nullptr, *z_scale = nullptr, *z_shift = nullptr;
  int z_ld = 0;
  // per forward call: the readers really go through z (set by dc_forward).  False — and `a` is written by the
  // BatchNorm + ReLU pass as on any other block — whenever a multiplier acts on the activated tensor in this call: a
  // caller-supplied Dropout2d mask on a block built with rate 0 (mimo_forward_args.drop_masks is honoured on every
  // block), or an element-wise final-dropout mask on a decoder output
  bool z_live = false;
};

struct ConvBN {
  std::string conv_name, bn_name;
  int Cin = 0, Cout = 0, cin_p = 0, cout_p = 0;
  int N = 0, H = 0, W = 0;
  ConvRecipe r;  // which kernels run this layer and on what packed rows, tiles and splits (conv_recipe.h)
  // the launches of the three directions, ready-made by fill_launches at the end of build(): a call copies one and sets what
  // varies per call
  ConvLaunch fwd, dgrad;
  WgradLaunch wgrad;
  BnReluLayer bn = {};  // what the BatchNorm + ReLU passes over z take, forward and backward (elementwise.h): fill_launches too
  int64_t off_w = 0, off_b = 0, off_gamma = 0, off_beta = 0, off_rm = 0, off_rv = 0;
  float *wf = nullptr, *wd = nullptr, *bias_p = nullptr;
  void *wf16 = nullptr, *wd16 = nullptr;  // split-bf16 packed weights (MIMO_PREC_SPLIT16)
  unsigned* wmax = nullptr;  // fp16 forward weight image: max |w| of the layer AT ITS LAST PACK, float bits (w16_scale: the image's power-of-two scale)
  int *cin_map = nullptr, *fwd_row_map = nullptr, *dg_row_map = nullptr, *dg_col_map = nullptr;
  float* z = nullptr;  // (element type: r.dtz)
  float *mean = nullptr, *invstd = nullptr, *scale = nullptr, *shift = nullptr, *c1 = nullptr, *c2 = nullptr;
  const float* in = nullptr;
  int ld_in = 0;
  float* a = nullptr;  // output activation
  int ld_a = 0;
  float* pool_out = nullptr;  // the MaxPool2d(2) of `a` is written by the BatchNorm + ReLU pass (training forward)
  int pool_ld = 0;
  // Second convolution of a DoubleConv whose loaders apply the first one's BatchNorm + ReLU themselves (round 4): forward and
  // weight gradient read the first convolution's pre-activation tensor `in_z` with its scale / shift, and the activated
  // tensor between the two convolutions (components.py:24-25) is never written.  `act_elided` marks that first convolution.
  bool fuse_in = false, act_elided = false;  // (act_elided on a second convolution: its readers apply it, see Act::z)
  const float* in_z = nullptr;
  int ld_in_z = 0;
  const float *in_scale = nullptr, *in_shift = nullptr;
};

enum InputKind { IN_IMAGE = 0, IN_POOL = 1, IN_UPCAT = 2 };

struct DoubleConv {
  std::string prefix;
  ConvBN c1, c2;
  InputKind kind = IN_IMAGE;
  int subnet = -1;       // for IN_IMAGE
  Act* src0 = nullptr;   // IN_POOL: pooled tensor; IN_UPCAT: skip
  Act* src1 = nullptr;   // IN_UPCAT: low-resolution tensor
  float* in_buf = nullptr;  // materialised input (packed image / pooled / concat)
  int in_ld = 0;
  bool pool_fused = false;     // IN_POOL: in_buf is written by the producers' BatchNorm + ReLU pass
  float* dxpad_own = nullptr;  // IN_UPCAT: private buffer of c1's padded-domain data gradient (holds the skip slice
                               // until the skip tensor's pool backward has read it)
  float* mid = nullptr;  // a1
  Act out;               // a2 (+ gradient)
  float drop_p = 0.f;
  const float* mask = nullptr;  // set per forward call
  int64_t p_begin = 0, p_end = 0;  // this block's parameters in the flat parameter / gradient buffers (floats)
};

struct Head {
  int s = 0;
  int64_t off_w = 0, off_b = 0;
};

// What one forward was called with and what was decided for it (mimo_forward): built once by mimo_plan::forward, handed down by
// const reference to the issuing functions, to prepare_forward in front of them and to record_forward behind them.  The
// pointers are the caller's on the eager route, the plan's staging copies on the graph routes (staged_call).
struct FwdCall {
  static constexpr int kMaxSites = 56;  // Dropout2d sites (one per DoubleConv) + 1 + S element-wise ones: checked by build()
  const float* x = nullptr;
  int64_t stride_n = 0, stride_s = 0;
  const int64_t* perm = nullptr;
  int64_t rows = 0;  // rows of x (= rows of the label / mask tensors of that batch)
  bool x5 = false, x4 = false;  // x is a dense [rows,S,Ci,H,W] / a dense [rows,Ci,H,W] shared by the subnetworks (stride_s = 0)
  float* out = nullptr;
  const float* masks[kMaxSites] = {};       // per DoubleConv: the Dropout2d multipliers in effect (the caller's or drawn in the engine)
  const float* elem_masks[kMaxSites] = {};  // [1 + S] the caller's element-wise multipliers (center, final[s])
  bool elem_rng_on[kMaxSites] = {};         // [1 + S] ... or drawn in the engine from (rng_seed, rng_offset)
  // element-wise dropout in this call, the caller's or the engine's: off the hipGraph routes (the caller's array may hold
  // nothing but null pointers and still counts; the generator state changes per call)
  bool elem_dropout = false;
  uint64_t rng_seed = 0, rng_offset = 0;
  bool training = false;
  bool no_grad = false;      // BN / ReLU folded into the conv epilogues, nothing saved for a backward (eval mode only)
  bool need_derive = true;   // (re)pack the weights and the eval BN constants in this forward
  int64_t version_after = -1;  // derived_version once the call has succeeded
  bool elem_on(int j) const { return elem_masks[j] || elem_rng_on[j]; }
};

// What one walk of the backward stages was called with (mimo_backward*, mimo_input_gradient): handed down by reference from
// backward_stage to the layer functions, nothing of it is kept on the plan.
struct BwdCall {
  const float *dout = nullptr, *dloss = nullptr;
  float* dx = nullptr;
  // mimo_input_gradient (evaluation-grade backward: the data-gradient chain only): a layer launches the BatchNorm-backward
  // apply pass and the data gradient and nothing else
  bool ig = false;
  float* dimage = nullptr;  // ... the image gradient [N,Ci,H,W] the encoders' first-layer data gradients are folded into
  bool accumulate = false;  // ... the first fold adds to what is there
  // mimo_input_gradient_mc: the plan batch holds `replicas` Monte-Carlo passes of N / replicas images, pass-major; dimage is
  // [N / replicas,Ci,H,W] and each encoder's fold sums its passes (0: mimo_input_gradient, dimage is [N,Ci,H,W])
  int replicas = 0;
};

// The dz buffers between the caller's stream (BatchNorm backward writes dz, the data gradient reads it) and the side stream
// (the weight gradient reads it): buffers, max |dz| slots, split copies and events, and every cross-stream wait / record of
// the protocol.  Which slot and which wait is decided by sched::DzRingPolicy (dz_ring.h, walked by tests/host/dz_ring_test.cpp).
struct DzRing {
  static constexpr int kSlots = sched::DzRingPolicy::kSlots;
  sched::DzRingPolicy policy;
  hipStream_t side = nullptr;  // the weight gradients' stream (null: everything on the caller's stream)
  hipEvent_t ev_dz[kSlots] = {}, ev_wg[kSlots] = {}, ev_join = nullptr;
  float* dz[kSlots] = {};
  float* dzmax[kSlots] = {};  // per-workgroup maxima of |dz| of the tensor in dz[i] (two-MFMA weight gradient)
  // split (bf16 hi|lo) copy of dz for layers whose data gradient runs on the fp32 kernel while the weight
  // gradient runs on the bf16-pair kernel (fewer than 16 output channels); null when no layer needs it
  float* dzs[kSlots] = {};
  // one layer's use of a slot, and what its BatchNorm backward left there for its weight gradient
  struct Slot {
    int b = 0, wait_on = -1;
    bool async = false, dz_on_launch = false;  // async: the weight gradient of this layer runs on the side stream
    const float* dz_wg = nullptr;  // dz as the weight gradient reads it (the split copy where one was made)
    float* absmax = nullptr;       // per-workgroup maxima of |dz| (two-MFMA weight gradient), absmax_n of them
    int absmax_n = 0;
  };
  ~DzRing() {
    if (side) (void)hipStreamDestroy(side);
    for (int i = 0; i < kSlots; ++i)
      for (hipEvent_t e : {ev_dz[i], ev_wg[i]})
        if (e) (void)hipEventDestroy(e);
    if (ev_join) (void)hipEventDestroy(ev_join);
  }
  // the slot the next layer writes (!async: the current one, nothing moves and nothing is waited for)
  Slot acquire(bool async) {
    Slot s;
    s.b = policy.next;
    s.async = async;
    if (async) s.wait_on = policy.acquire().wait_on;
    return s;
  }
  // in front of the launch that overwrites dz[s.b] and dzmax[s.b] on `st`
  int wait_free(const Slot& s, hipStream_t st) {
    if (s.wait_on >= 0) MIMO_HIP_CHECK(hipStreamWaitEvent(st, ev_wg[s.wait_on], 0));
    return MIMO_OK;
  }
  // "dz exists" travels with the launch that writes it (a stop event on the kernel, no hipEventRecord behind it) whenever that
  // launch is the last writer — not when a split copy of dz follows — and not under stream capture
  hipEvent_t dz_event_on_launch(Slot& s, bool capturing, bool split_copy_follows) {
    s.dz_on_launch = s.async && !capturing && !split_copy_follows;
    return s.dz_on_launch ? ev_dz[s.b] : nullptr;
  }
  // behind the last writer of dz on `st`: wgrad(L) may start as soon as dz exists, next to dgrad(L)
  int dz_written(const Slot& s, hipStream_t st) {
    if (s.async && !s.dz_on_launch) MIMO_HIP_CHECK(hipEventRecord(ev_dz[s.b], st));
    return MIMO_OK;
  }
  // the stream the weight gradient of this layer runs on, made to wait for dz
  int reader_stream(const Slot& s, hipStream_t st, hipStream_t* ws) {
    *ws = st;
    if (s.async) {
      MIMO_HIP_CHECK(hipStreamWaitEvent(side, ev_dz[s.b], 0));  // (a wait refers to the record made just above)
      *ws = side;
    }
    return MIMO_OK;
  }
  // the release event travels with the weight gradient's reduction launch, unless there is none (thin: the plain-FMA kernel's
  // launch reduces its own partials) or the stream is being captured
  hipEvent_t release_on_launch(const Slot& s, bool capturing, bool thin) const {
    return (s.async && !capturing && !thin) ? ev_wg[s.b] : nullptr;
  }
  // dz buffer b AND its max |dz| slots are free again — recorded behind the REDUCTION: it reads the slots too (to take the
  // two-MFMA kernel's scale out again), and the BatchNorm backward of the layer after next overwrites them.  (Until the
  // end of round 5 the event sat in front of the reduction: a race that showed as a weight gradient off by > 1e-4 of
  // its scale in one small-geometry test when that test ran alone.)
  int released(const Slot& s, bool rode_on_launch) {
    if (!s.async) return MIMO_OK;
    if (!rode_on_launch) MIMO_HIP_CHECK(hipEventRecord(ev_wg[s.b], side));
    policy.released(s.b);
    return MIMO_OK;
  }
  // the caller's stream waits for every weight gradient issued so far
  int join(hipStream_t st) {
    if (!side || !policy.any_pending()) return MIMO_OK;
    MIMO_HIP_CHECK(hipEventRecord(ev_join, side));
    MIMO_HIP_CHECK(hipStreamWaitEvent(st, ev_join, 0));
    policy.joined();
    return MIMO_OK;
  }
};

// Optional per-kernel-class timing with HIP events on the launch stream (bench.py roofline, mimo_plan_profile*).
struct Profiler {
  struct Rec {
    hipEvent_t a, b;
    int kind, tier;
  };
  // tier records: kind = kTierBase + 2 * tier + (backward ? 1 : 0); tier = resolution level of a DoubleConv
  // (0 = full resolution ... 4 = 1/16): the whole block (every launch between the two events), so that a tier's
  // summed device time can be priced against its algorithmic HBM bytes
  static constexpr int kTierBase = 100, kTiers = 5;
  bool on = false;
  int cur_tier = 0;  // resolution tier of the block being issued (kernel-class records inherit it)
  std::vector<Rec> recs;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pool;
  double ms[MIMO_PROF_KINDS] = {}, flops[MIMO_PROF_KINDS] = {}, bytes[MIMO_PROF_KINDS] = {};
  int64_t launches[MIMO_PROF_KINDS] = {};
  double kind_tier_ms[MIMO_PROF_KINDS][kTiers] = {};
  double tier_ms[2 * kTiers] = {};
  // (runs behind ~mimo_plan's body — buffers freed, graphs, cap_stream and ev_stage destroyed — and in front of ~DzRing;
  // these events are recorded on the caller's streams only and destroying them needs none of those)
  ~Profiler() {
    for (auto& r : recs) {
      (void)hipEventDestroy(r.a);
      (void)hipEventDestroy(r.b);
    }
    for (auto& e : pool) {
      (void)hipEventDestroy(e.first);
      (void)hipEventDestroy(e.second);
    }
  }
  int begin(int kind, hipStream_t st) {
    if (!on) return -1;
    Rec r;
    if (!pool.empty()) {
      r.a = pool.back().first;
      r.b = pool.back().second;
      pool.pop_back();
    } else {
      (void)hipEventCreate(&r.a);
      (void)hipEventCreate(&r.b);
    }
    r.kind = kind;
    if (kind >= kTierBase) cur_tier = (kind - kTierBase) / 2;
    r.tier = cur_tier;
    (void)hipEventRecord(r.a, st);
    recs.push_back(r);
    return (int)recs.size() - 1;
  }
  void end(int idx, double fl, double by, hipStream_t st) {
    if (idx < 0 || !on) return;
    (void)hipEventRecord(recs[idx].b, st);
    const int kind = recs[idx].kind;
    if (kind >= kTierBase) return;
    flops[kind] += fl;
    bytes[kind] += by;
    launches[kind] += 1;
  }
  int collect() {
    for (auto& r : recs) {
      MIMO_HIP_CHECK(hipEventSynchronize(r.b));
      float t = 0.f;
      MIMO_HIP_CHECK(hipEventElapsedTime(&t, r.a, r.b));
      if (r.kind >= kTierBase)
        tier_ms[r.kind - kTierBase] += t;
      else {
        ms[r.kind] += t;
        kind_tier_ms[r.kind][r.tier] += t;
      }
      pool.emplace_back(r.a, r.b);
    }
    recs.clear();
    return MIMO_OK;
  }
  void clear_totals() {
    for (int k = 0; k < MIMO_PROF_KINDS; ++k) {
      ms[k] = flops[k] = bytes[k] = 0.0;
      launches[k] = 0;
    }
    for (double& v : tier_ms) v = 0.0;
    for (auto& row : kind_tier_ms)
      for (double& v : row) v = 0.0;
  }
};

}  // namespace
}  // namespace mimo

using namespace mimo;

struct mimo_plan {
  mimo_config cfg;
  int S, f, N, H, W, Ci, Co, Ci_p;
  // 16-bit storage modes (MIMO_PREC_BF16_MIXED / MIMO_PREC_FP16_MIXED): activations, conv outputs and their gradients
  // live in HBM as bf16 / fp16 (st, esz bytes per element); every "float*" of such a tensor is then an untyped byte
  // address and channel offsets go through eoff()
  bool mixed = false, f16 = false;
  int st = ST_F32, esz = 4;
  float* eoff(float* p, size_t elems) const { return reinterpret_cast<float*>(reinterpret_cast<char*>(p) + elems * esz); }
  int alloc_act(float** p, size_t elems, int dt) {  // activation-like tensor of `elems` elements of StoreType dt
    return dalloc(p, (elems * store_bytes(dt) + 3) / 4);
  }
  int fwd_mode() const { return pack::conv_mode(cfg.precision, PACK_FWD); }  // conv3x3_bf16x3_launch modes
  int dgrad_mode() const { return pack::conv_mode(cfg.precision, PACK_DGRAD); }
  std::vector<TensorInfo> tensors;
  int64_t param_floats = 0, buffer_floats = 0;
  float *params = nullptr, *grads = nullptr, *bnbuf = nullptr;
  std::vector<void*> allocs;
  size_t bytes = 0;

  std::vector<std::unique_ptr<DoubleConv>> dcs;  // forward order == oracle double_conv_specs
  std::vector<DoubleConv*> enc_in, down1, up4;
  DoubleConv *down2 = nullptr, *down3 = nullptr, *down4 = nullptr, *up1 = nullptr, *up2 = nullptr, *up3 = nullptr;
  Act x2cat;  // concat of the S encoder outputs (model.py:113)
  std::vector<Head> heads;

  // scratch
  float *s_dz = nullptr, *s_dxpadA = nullptr, *s_dxpadB = nullptr, *s_wslab = nullptr,
        *s_partial = nullptr, *s_losspart = nullptr;
  float* s_headpart = nullptr;  // GS_HEAD: the head's weight / bias gradient partial rows, written by the BatchNorm-backward reduction
  int head_rows = 0;            // ... and how many (that launch's grid)
  double* s_sums = nullptr;  // rowsum_launch's chunk sums (convolution epilogues with more than kColsumMaxRows partial rows)
  int* d_status = nullptr;  // numerics status word (mimo_plan_status)
  size_t cap_act = 0, cap_pad = 0, cap_slab = 0, cap_partial = 0, cap_sums = 0;
  float* s_kpart = nullptr;  // partial-sum slabs of the K-split convolution launches (conv3x3_bf16x3_launch_k)
  size_t cap_kpart = 0;

  // MIMO_WGRAD_STREAM (default 1): weight gradients on a side stream — wgrad(L) (matrix-pipe bound, little HBM
  // traffic) overlaps the bandwidth-bound BatchNorm / gather kernels of the layers below it on the caller's stream;
  // dz goes round the buffers of `ring` so that the layers below L can write their dz while wgrad(L) still reads its own.
  // (Measured and removed in round 3: per-layer dz buffers without back-pressure, 3-4 ping-pong buffers with a wait per
  // layer, releasing a weight gradient only after its layer's data gradient — none faster)
  bool wg_async = false;
  // the switches and the device as conv_recipe takes them, read once by build(); env.wg_cus: the CUs the weight-gradient launches
  // are sized for (sched::wg_side_cus; MIMO_WGRAD_CUS overrides)
  ConvEnv env;
  // test hook (MIMO_DEBUG_WGRAD_DELAY_US, read per plan): an idle kernel of that many microseconds in front of every weight
  // gradient, on the stream it runs on — the consumer of dz and its max |dz| slots arrives late (tests/test_streams_gpu.py)
  int wg_delay_us = 0;
  // BatchNorm backward forms the gradient arriving at a pooled tensor / at the head's input itself (GS_POOL / GS_HEAD):
  // fp32 storage, MIMO_FUSE_BWD_SRC=0 switches it off (read per plan)
  bool fuse_bwd_src = false;
  // BatchNorm + ReLU applied by the readers of a tensor instead of a pass of its own (ConvBN::fuse_in, Act::z):
  // MIMO_FUSE_BN_IN=0 materialises every activated tensor (read per plan: A/B, tests)
  bool fuse_bn_in = true;
  bool fuse_bwd_pool = false, fuse_bwd_head = false;  // (MIMO_FUSE_BWD_SRC=2: pooled tensors only, 3: head only — A/B)
  DzRing ring;  // dz buffers, their events and the side stream (ring.side)
  hipEvent_t ev_stage = nullptr;
  bool any_mixed_dz = false;

  Profiler prof;
  int tier_of(int h) const {  // resolution tier of a block at height h (Profiler::kTierBase records)
    int t = 0, hh = H;
    while (t < Profiler::kTiers - 1 && hh > h) {
      hh /= 2;
      ++t;
    }
    return t;
  }

  // hipGraph replay of the eval-mode forward (launch-bound at small batch: ~100+ kernel launches).
  // The captured kernels read plan-owned staging copies of x / perm / masks and write a plan-owned
  // logits buffer, so the graph stays valid when the caller's tensors move.
  // Whether a graphable call runs eagerly, is captured or replays what is live is decided by sched::GraphReplayPolicy
  // (graph_replay.h, walked by tests/host/graph_replay_test.cpp), one per route; the handles, capture(), the staging copies and
  // the "is this call graphable" predicates are here.  The eval-mode route captures a call shape at first sight.
  bool graph_enabled = true;
  hipStream_t cap_stream = nullptr;
  hipGraphExec_t graph_exec = nullptr;
  sched::GraphReplayPolicy eval_replay = sched::GraphReplayPolicy::eval_forward();
  // hipGraph replay of the TRAINING step (round 6, MIMO_TRAIN_GRAPH=1, opt-in; mimo_unet.py:115-144 at its per-GPU shard is ~290
  // launches of which ~200 run < 20 us): the training forward is one graph, the backward one graph (mimo_backward) or one
  // per stage (mimo_backward_stage: the data-parallel caller starts a stage's all-reduce between two graphs).  Captured
  // kernels only see plan-owned memory: x / perm / Dropout2d multipliers are staged in front of the forward graph, label /
  // mask / perm by mimo_loss_forward, dloss in front of the first backward graph, the logits leave through g_out.  A call
  // shape (key) is captured the SECOND time it is seen — one-off shapes stay eager, and every kernel has run eagerly once
  // before it is captured (tg_fwd_replay / tg_bwd_replay) — out of one budget of captures per plan: a caller that keeps
  // alternating call shapes on one plan would otherwise re-capture (milliseconds of host time) every other step.  The side
  // stream's weight gradients are a fork / join inside each backward graph.
  bool train_graph = false;
  hipGraphExec_t tg_fwd = nullptr;
  static constexpr int kBwdGraphs = 9;  // [0, 8): the single stages; [8]: the whole backward
  hipGraphExec_t tg_bwd[kBwdGraphs] = {};
  sched::CaptureBudget tg_budget{/*max=*/24};
  sched::GraphReplayPolicy tg_fwd_replay = sched::GraphReplayPolicy::training_forward(&tg_budget);
  sched::GraphReplayPolicy tg_bwd_replay = sched::GraphReplayPolicy::training_backward(&tg_budget);
  bool tg_bwd_live = false;    // the backward in progress replays graphs (decided at its stage 0)
  float *g_label = nullptr, *g_lmask = nullptr, *g_dloss = nullptr;
  int64_t* g_lperm = nullptr;
  static void destroy_exec(hipGraphExec_t* e) {
    if (*e) (void)hipGraphExecDestroy(*e);
    *e = nullptr;
  }
  void drop_graphs() {  // (spent captures are not refunded)
    destroy_exec(&graph_exec);
    eval_replay.reset();
    destroy_exec(&tg_fwd);
    tg_fwd_replay.reset();
    for (auto& e : tg_bwd) destroy_exec(&e);
    tg_bwd_replay.reset();
  }
  float *g_x = nullptr, *g_out = nullptr;
  int64_t* g_perm = nullptr;
  std::vector<float*> g_masks;
  // in-engine dropout (mimo_forward_args.rng_sites): Dropout2d multipliers are drawn into g_masks by one Philox
  // launch per forward; the element-wise sites (center / final nn.Dropout) regenerate theirs on the fly in the
  // forward and in the backward from the (seed, offset) of the last forward
  Dropout2dSite* d_sites = nullptr;
  int max_site_count = 0;
  float elem_rate(int j) const { return j == 0 ? cfg.center_dropout_rate : cfg.final_dropout_rate; }
  ElemRng elem_rng(int j, uint64_t seed, uint64_t offset) const { return ElemRng{seed, offset, (int)dcs.size() + j, elem_rate(j)}; }
  ElemRng elem_rng(int j) const { return elem_rng(j, rng_seed, rng_offset); }  // of the last forward

  bool capturing = false;

  // max |w| words of the fp16 forward weight images (ConvBN::wmax), one array: zeroed and re-taken by every pack, so that a
  // transient huge weight (a diverged step followed by load_state_dict) does not leave a layer's image at a tiny scale
  static constexpr int kMaxWmaxWords = 128;
  unsigned* wmax_pool = nullptr;
  int wmax_used = 0;
  // weight repack job tables (device): [0, n_fwd_jobs) forward packs (+ bias copies), then the data-gradient packs
  PackJob* pack_jobs = nullptr;
  int n_fwd_jobs = 0, n_all_jobs = 0, pack_max_total = 0;

  // What the last forward left for the loss and the backward: assigned by record_forward.  (Besides: forward() ends
  // fwd_graphed / loss_staged at once, mimo_loss_forward sets loss_done / loss_staged, a failed forward and mimo_plan_bind reset
  // derived_version.)  dcs[i]->mask and Act::z_live belong to it and are set by prepare_forward.
  bool fwd_done = false, fwd_training = false, had_perm = false, loss_done = false;
  bool fwd_no_grad = false;       // last forward folded BN/ReLU into the conv epilogue: nothing saved for a backward
  float* out = nullptr;
  std::vector<const float*> elem_masks;  // [1 + S] element-wise dropout multipliers of the last forward
  std::vector<char> elem_rng_on;         // [1 + S] ... drawn in the engine, from:
  uint64_t rng_seed = 0, rng_offset = 0;
  bool fwd_graphed = false;    // the last forward was a training-graph replay: logits in g_out, masks staged
  bool loss_staged = false;    // ... and mimo_loss_forward staged label / mask / perm
  int64_t last_x_rows = 0;     // rows of the last forward's x (= rows of the label / mask tensors of that batch)
  const int64_t* last_perm_arg = nullptr;  // the caller's perm tensor of the last graphed forward (staged in g_perm)
  int64_t derived_version = -1;   // param_version the packed weights / eval scale+shift were derived from (-1: none)

  int bwd_next_stage = 0;  // staged backward: the stage that may run next (0 = a fresh backward)
  int64_t encoder_param_floats = 0;
  float* s_zero = nullptr;        // max cout_p zeros, never written: c1 / c2 of the apply pass after an eval-mode forward
  size_t cap_cout = 0;
  int64_t dgrad_version = -1;     // derived_version the data-gradient weight images were packed at by mimo_input_gradient (-1: none)
  const float *label = nullptr, *lmask = nullptr;  // of the last mimo_loss_forward
  const int64_t* lperm = nullptr;

  ~mimo_plan() {
    for (void* p : allocs) (void)hipFree(p);
    drop_graphs();
    if (cap_stream) (void)hipStreamDestroy(cap_stream);
    if (ev_stage) (void)hipEventDestroy(ev_stage);
  }

  template <typename T>
  int dalloc(T** p, size_t count) {
    void* q = nullptr;
    const size_t nbytes = std::max<size_t>(count, 1) * sizeof(T);
    MIMO_HIP_CHECK(hipMalloc(&q, nbytes));
    MIMO_HIP_CHECK(hipMemset(q, 0, nbytes));
    allocs.push_back(q);
    bytes += nbytes;
    *p = static_cast<T*>(q);
    return MIMO_OK;
  }
  int upload_ints(int** p, const std::vector<int>& v) {
    MIMO_TRY(dalloc(p, v.size()));
    MIMO_HIP_CHECK(hipMemcpy(*p, v.data(), v.size() * sizeof(int), hipMemcpyHostToDevice));
    return MIMO_OK;
  }

  int64_t add_tensor(const std::string& name, std::vector<int64_t> shape, int kind) {
    TensorInfo t;
    t.name = name;
    t.ndim = (int)shape.size();
    int64_t n = 1;
    for (int i = 0; i < 4; ++i) {
      t.shape[i] = i < t.ndim ? shape[i] : 1;
      n *= t.shape[i];
    }
    t.kind = kind;
    int64_t& cur = kind == 0 ? param_floats : buffer_floats;
    t.offset = cur;
    cur += (n + 3) / 4 * 4;  // keep every tensor 16-byte aligned inside the flat buffers
    tensors.push_back(t);
    return t.offset;
  }

  // A layer in three steps: what it runs (conv_recipe), its parameters, its buffers and its share of the scratch capacities
  int init_convbn(ConvBN& L, const std::string& prefix, int conv_idx, int bn_idx, int Cin, int Cout,
                  const std::vector<int>& in_chmap, int n, int h, int w) {
    L.conv_name = prefix + "." + std::to_string(conv_idx);
    L.bn_name = prefix + "." + std::to_string(bn_idx);
    L.Cin = Cin;
    L.Cout = Cout;
    L.cin_p = (int)in_chmap.size();
    L.cout_p = pad_channels(Cout);
    L.N = n;
    L.H = h;
    L.W = w;
    bool ident = true;  // (the packed image: logical channel i in padded channel i)
    for (int i = 0; i < Cin; ++i) ident = ident && i < L.cin_p && in_chmap[i] == i;
    L.r = conv_recipe(cfg.precision, cfg.inference_only, n, h, w, Cin, Cout, L.cin_p, L.cout_p, ident, env);
    register_convbn(L);
    return alloc_convbn(L, in_chmap);
  }

  void register_convbn(ConvBN& L) {
    L.off_w = add_tensor(L.conv_name + ".weight", {L.Cout, L.Cin, 3, 3}, 0);
    L.off_b = add_tensor(L.conv_name + ".bias", {L.Cout}, 0);
    L.off_gamma = add_tensor(L.bn_name + ".weight", {L.Cout}, 0);
    L.off_beta = add_tensor(L.bn_name + ".bias", {L.Cout}, 0);
    L.off_rm = add_tensor(L.bn_name + ".running_mean", {L.Cout}, 1);
    L.off_rv = add_tensor(L.bn_name + ".running_var", {L.Cout}, 1);
  }

  int alloc_convbn(ConvBN& L, const std::vector<int>& in_chmap) {
    const ConvRecipe& r = L.r;
    const int n = L.N, h = L.H, w = L.W;
    const bool train_bufs = cfg.inference_only != 1;  // everything only a backward reads or writes
    const bool wgrad_bufs = cfg.inference_only == 0;  // ... only a weight gradient (inference_only = 2: input gradient only)
    MIMO_TRY(dalloc(&L.wf, pack::image_elems(PK_F32, r.fwd.rows, L.cin_p)));
    if (train_bufs) MIMO_TRY(dalloc(&L.wd, pack::image_elems(PK_F32, r.dgrad.rows, L.cout_p)));
    MIMO_TRY(dalloc(&L.bias_p, r.fwd.rows));
    if (r.thin && wgrad_bufs) cap_slab = std::max(cap_slab, wgrad_thin_scratch(L.Cin, L.cout_p));
    if (r.wg_split && !r.dgrad.split) any_mixed_dz = true;
    cap_kpart = std::max(cap_kpart, std::max(r.fwd.kpart, r.dgrad.kpart));  // the slabs of the K-split launches
    if (r.fwd.split && (cfg.precision == MIMO_PREC_SPLIT16 || cfg.precision == MIMO_PREC_FP16_MIXED)) {
      // one array for all layers' words: every pack zeroes it in one memset and takes the maxima afresh (pack_all)
      if (!wmax_pool) MIMO_TRY(dalloc(&wmax_pool, kMaxWmaxWords));
      if (wmax_used >= kMaxWmaxWords) {
        set_error("too many convolution layers (%d) for the fp16 weight-scale words", wmax_used + 1);
        return MIMO_ERR_INVALID;
      }
      L.wmax = wmax_pool + wmax_used++;
    }
    if (r.fwd.split) {
      uint16_t* q = nullptr;
      MIMO_TRY(dalloc(&q, pack::image_elems(pack::kind(cfg.precision, PACK_FWD, true, r.fwd.wide != 0),
                                            r.fwd.wide ? r.fwd.wide : r.fwd.rows, L.cin_p)));
      L.wf16 = q;
    }
    if (r.dgrad.split && train_bufs) {
      uint16_t* q = nullptr;
      MIMO_TRY(dalloc(&q, pack::image_elems(pack::kind(cfg.precision, PACK_DGRAD, true, r.dgrad.wide != 0),
                                            r.dgrad.wide ? r.dgrad.wide : r.dgrad.rows, L.cout_p)));
      L.wd16 = q;
    }
    MIMO_TRY(upload_ints(&L.cin_map, in_chmap));
    std::vector<int> frm(r.fwd.rows), drm(r.dgrad.rows), dcm(L.cout_p);
    for (int i = 0; i < r.fwd.rows; ++i) frm[i] = i < L.Cout ? i : -1;
    for (int i = 0; i < r.dgrad.rows; ++i) drm[i] = i < L.cin_p ? in_chmap[i] : -1;
    for (int i = 0; i < L.cout_p; ++i) dcm[i] = i < L.Cout ? i : -1;
    MIMO_TRY(upload_ints(&L.fwd_row_map, frm));
    MIMO_TRY(upload_ints(&L.dg_row_map, drm));
    MIMO_TRY(upload_ints(&L.dg_col_map, dcm));
    // (16-bit storage: the image convolution runs on the fp32 kernels and always goes through an fp32 z)
    if (train_bufs || (mixed && !r.fwd.split)) MIMO_TRY(alloc_act(&L.z, (size_t)n * h * w * L.cout_p, r.dtz));
    MIMO_TRY(dalloc(&L.mean, L.cout_p));
    MIMO_TRY(dalloc(&L.invstd, L.cout_p));
    MIMO_TRY(dalloc(&L.scale, L.cout_p + kFinSlack));  // (+ zero slack: the next convolution's loaders read whole K chunks)
    MIMO_TRY(dalloc(&L.shift, L.cout_p + kFinSlack));
    MIMO_TRY(dalloc(&L.c1, L.cout_p));
    MIMO_TRY(dalloc(&L.c2, L.cout_p));
    cap_act = std::max(cap_act, (size_t)n * h * w * L.cout_p);
    cap_pad = std::max(cap_pad, (size_t)n * (h + 2) * (w + 2) * L.cin_p);
    cap_cout = std::max(cap_cout, (size_t)L.cout_p);
    // slabs + the reduction's group-sum levels (geometric: < splits/15 extra slabs)
    cap_slab = std::max(cap_slab, (size_t)(r.wg_splits + r.wg_splits / 8 + 2) * 9 * r.wg_cin_pad * r.wg_cout_pad);
    const size_t stat_rows = std::max(conv3x3_stat_rows(n, h, w), conv3x3_ws_stat_rows(n, h, w));
    cap_partial = std::max(cap_partial, stat_rows * 2 * r.fwd.rows);
    cap_partial = std::max(cap_partial, (size_t)kBnReduceMaxBlocks * 2 * L.cout_p);
    cap_sums = std::max(cap_sums, (size_t)kMaxChunks * 2 * round_up(std::max(r.fwd.rows, L.cout_p), 64));
    return MIMO_OK;
  }

  // The ready-made launches of a layer, once build() has settled where its tensors live (rehome_skip, elide_output, the pool fusion)
  void fill_launches(ConvBN& L) {
    L.fwd = fill_conv_launch(L.r, PACK_FWD, L.N, L.H, L.W, L.cin_p, L.cout_p);
    L.fwd.x = L.in;
    L.fwd.ldx = L.ld_in;
    L.fwd.y = L.z;
    L.fwd.w = L.wf;
    L.fwd.wpk = L.wf16;
    L.fwd.bias = L.bias_p;
    L.fwd.wmax = L.wmax;
    L.dgrad = fill_conv_launch(L.r, PACK_DGRAD, L.N, L.H, L.W, L.cin_p, L.cout_p);
    L.dgrad.w = L.wd;
    L.dgrad.wpk = L.wd16;
    L.wgrad = fill_wgrad_launch(L.r, L.N, L.H, L.W, L.cin_p, L.cout_p);
    L.wgrad.x = L.fuse_in ? L.in_z : L.in;
    L.wgrad.ldx = L.fuse_in ? L.ld_in_z : L.ld_in;
    L.wgrad.in_scale = L.in_scale;  // (null without fuse_in)
    L.wgrad.in_shift = L.in_shift;
    L.wgrad.partial = s_wslab;
    L.bn = BnReluLayer{L.z, L.r.dtz, L.cout_p, st, L.scale, L.shift, L.mean, L.invstd, L.Cout, L.cout_p, L.N, L.H, L.W};
  }

  // Create a DoubleConv whose input has channel map in_chmap at resolution (h, w).
  int make_dc(DoubleConv** outp, const std::string& prefix, const std::vector<int>& in_chmap, int Cin, int Cmid,
              int Cout, int h, int w, float drop_p, float* out_a, int out_ld, float* out_da, int out_ldda) {
    auto dc = std::make_unique<DoubleConv>();
    dc->prefix = prefix;
    dc->drop_p = drop_p;
    dc->p_begin = param_floats;
    MIMO_TRY(init_convbn(dc->c1, prefix, 0, 1, Cin, Cmid, in_chmap, N, h, w));
    std::vector<int> midmap(pad_channels(Cmid));
    for (size_t i = 0; i < midmap.size(); ++i) midmap[i] = (int)i < Cmid ? (int)i : -1;
    MIMO_TRY(init_convbn(dc->c2, prefix, 3, 4, Cmid, Cout, midmap, N, h, w));
    dc->p_end = param_floats;
    MIMO_TRY(alloc_act(&dc->mid, (size_t)N * h * w * dc->c1.cout_p, st));
    Act& o = dc->out;
    o.N = N;
    o.H = h;
    o.W = w;
    o.C = Cout;
    o.Cp = dc->c2.cout_p;
    o.chmap.resize(o.Cp);
    for (int i = 0; i < o.Cp; ++i) o.chmap[i] = i < Cout ? i : -1;
    if (out_a) {
      o.a = out_a;
      o.ld = out_ld;
      o.da = out_da;
      o.ldda = out_ldda;
    } else {
      MIMO_TRY(alloc_act(&o.a, (size_t)N * h * w * o.Cp, st));
      if (cfg.inference_only != 1) MIMO_TRY(alloc_act(&o.da, (size_t)N * h * w * o.Cp, st));
      o.ld = o.ldda = o.Cp;
    }
    dc->c1.a = dc->mid;
    dc->c1.ld_a = dc->c1.cout_p;
    dc->c2.in = dc->mid;
    dc->c2.ld_in = dc->c1.cout_p;
    {
      // BatchNorm + ReLU of the first convolution applied by the second one's loaders: split16, when BOTH readers of the
      // activated tensor — the second convolution's forward and its weight gradient — run on kernels that can (the
      // wide / 256-pixel wave-specialised forward, the wave-specialised weight gradient).  MIMO_FUSE_BN_IN=0: materialise.
      ConvBN& c2 = dc->c2;
      if (fuse_bn_in && cfg.precision == MIMO_PREC_SPLIT16 && !cfg.inference_only && c2.r.fwd.split && c2.r.wg_split && dc->c1.r.dtz == ST_F32 &&
          conv3x3_split_fuses_input(fwd_mode(), c2.r.fwd.wide, h, w) && wgrad_split_fuses_input(c2.cin_p, c2.cout_p, 0, 3)) {
        c2.fuse_in = true;
        c2.in_z = dc->c1.z;
        c2.ld_in_z = dc->c1.cout_p;
        c2.in_scale = dc->c1.scale;
        c2.in_shift = dc->c1.shift;
        dc->c1.act_elided = true;
      }
    }
    dc->c2.a = o.a;
    dc->c2.ld_a = o.ld;
    *outp = dc.get();
    dcs.push_back(std::move(dc));
    return MIMO_OK;
  }

  // Skip connections cost no copy: the skip tensor is re-homed into channels [0, Cs) of the concat buffer of
  // the Up block that consumes it (its producers write it there with the concat's pixel pitch), so the
  // up-sample + concat kernel only writes the up-sampled channels.  `producers`: the ConvBN layers whose `a`
  // is (a channel slice of) this tensor, with their channel offsets.
  void rehome_skip(Act& sk, DoubleConv* up, std::vector<std::pair<DoubleConv*, int>> producers) {
    sk.a = up->in_buf;
    sk.ld = up->in_ld;
    for (auto& pr : producers) {
      DoubleConv* dc = pr.first;
      dc->c2.a = eoff(up->in_buf, pr.second);
      dc->c2.ld_a = up->in_ld;
      dc->out.a = dc->c2.a;
      dc->out.ld = up->in_ld;
    }
  }

  int set_input(DoubleConv* dc, InputKind kind, Act* s0, Act* s1, int in_cp, int h, int w) {
    dc->kind = kind;
    dc->src0 = s0;
    dc->src1 = s1;
    MIMO_TRY(alloc_act(&dc->in_buf, (size_t)N * h * w * in_cp, kind == IN_IMAGE ? ST_F32 : st));  // the packed image stays fp32
    // the skip slice of the data gradient stays in this block's own buffer until the pool backward of the skip tensor folds
    // it in (every skip tensor is pooled by a Down block)
    if (kind == IN_UPCAT && cfg.inference_only != 1)
      MIMO_TRY(alloc_act(&dc->dxpad_own, (size_t)N * (h + 2) * (w + 2) * in_cp, st));
    // the pooled gradient stays in this block's own buffer until the producers' BatchNorm backward has routed it (GS_POOL)
    if (kind == IN_POOL && fuse_bwd_pool) MIMO_TRY(alloc_act(&dc->dxpad_own, (size_t)N * (h + 2) * (w + 2) * in_cp, st));
    dc->in_ld = in_cp;
    dc->c1.in = dc->in_buf;
    dc->c1.ld_in = in_cp;
    return MIMO_OK;
  }

  static std::vector<int> cat_map(const Act& a, const Act& b) {
    std::vector<int> m = a.chmap;
    for (int v : b.chmap) m.push_back(v < 0 ? -1 : v + a.C);
    return m;
  }

  int build() {
    // 0: full plan; 2: input gradient only (mimo_input_gradient); any other value: 1, no backward at all
    if (cfg.inference_only != 0 && cfg.inference_only != 2) cfg.inference_only = 1;
    if (cfg.inference_only == 2 && cfg.precision != MIMO_PREC_FP32 && cfg.precision != MIMO_PREC_SPLIT16) {
      set_error("inference_only = 2 (input gradient only) exists for the fp32 and split16 precisions, not for precision %d", cfg.precision);
      return MIMO_ERR_INVALID;
    }
    mixed = pack::is_mixed(cfg.precision);
    f16 = cfg.precision == MIMO_PREC_FP16_MIXED;
    st = pack::store_type(cfg.precision);
    esz = store_bytes(st);
    {
      const int v = getenv("MIMO_FUSE_BWD_SRC") ? atoi(getenv("MIMO_FUSE_BWD_SRC")) : 1;
      // (an input-gradient-only plan routes the gradients exactly as a full plan does: the same bits)
      fuse_bwd_src = !mixed && cfg.inference_only != 1 && v != 0;
      fuse_bwd_pool = fuse_bwd_src && v != 3;
      fuse_bwd_head = fuse_bwd_src && v != 2;
      fuse_bn_in = !(getenv("MIMO_FUSE_BN_IN") && atoi(getenv("MIMO_FUSE_BN_IN")) == 0);
    }
    if (cfg.precision < MIMO_PREC_FP32 || cfg.precision > MIMO_PREC_FP16_MIXED) {
      set_error("unknown precision %d", cfg.precision);
      return MIMO_ERR_INVALID;
    }
    if (cfg.norm_kind != MIMO_NORM_BATCH || cfg.act_kind != MIMO_ACT_RELU || cfg.up_kind != MIMO_UP_BILINEAR_ALIGN_CORNERS) {
      set_error("block variant norm %d / act %d / up %d is not implemented: only BatchNorm2d + ReLU + bilinear align_corners "
                "up-sampling, the reference's blocks (components.py:22-30, 77-85)", cfg.norm_kind, cfg.act_kind, cfg.up_kind);
      return MIMO_ERR_INVALID;
    }
    S = cfg.num_subnetworks;
    f = cfg.filter_base_count;
    N = cfg.batch;
    H = cfg.height;
    W = cfg.width;
    Ci = cfg.in_channels;
    Co = cfg.out_channels;
    Ci_p = round_up(Ci, 4);
    {
      // (a property of the plan, not of the stream mode: MIMO_WGRAD_STREAM=0 and the profiler's serialised pass run the same
      // launches, so the two modes stay bit-identical)
      env = conv_env(wgrad_cus(sched::wg_side_cus((long)N * H * W, S * f)));
      const char* d = getenv("MIMO_DEBUG_WGRAD_DELAY_US");
      wg_delay_us = d ? std::max(0, std::min(atoi(d), 5000)) : 0;
    }
    if (S < 1 || f < 1 || N < 1 || Ci < 1 || Co < 2 || (Co & 1) || Co > kMaxHeadOut || f > 256) {
      set_error("unsupported configuration S=%d f=%d N=%d Ci=%d Co=%d", S, f, N, Ci, Co);
      return MIMO_ERR_INVALID;
    }
    if ((H >> 4) < 2 || (W >> 4) < 2) {
      set_error("input %dx%d too small: reflect padding needs >= 2 pixels at 1/16 resolution", H, W);
      return MIMO_ERR_INVALID;
    }
    const int H1 = H, W1 = W, H2 = H / 2, W2 = W / 2, H3 = H2 / 2, W3 = W2 / 2, H4 = H3 / 2, W4 = W3 / 2, H5 = H4 / 2,
              W5 = W4 / 2;
    std::vector<int> imgmap(Ci_p);
    for (int i = 0; i < Ci_p; ++i) imgmap[i] = i < Ci ? i : -1;

    // ---- encoder (model.py:150-175) ----
    for (int s = 0; s < S; ++s) {
      DoubleConv* dc;
      MIMO_TRY(make_dc(&dc, "encoder.in_convs." + std::to_string(s) + ".double_conv", imgmap, Ci, f, f, H1, W1,
                       cfg.encoder_dropout_rate, nullptr, 0, nullptr, 0));
      MIMO_TRY(set_input(dc, IN_IMAGE, nullptr, nullptr, Ci_p, H1, W1));
      dc->subnet = s;
      enc_in.push_back(dc);
    }
    const int c2p = pad_channels(2 * f);
    x2cat.N = N;
    x2cat.H = H2;
    x2cat.W = W2;
    x2cat.C = 2 * f * S;
    x2cat.Cp = c2p * S;
    x2cat.ld = x2cat.ldda = x2cat.Cp;
    MIMO_TRY(alloc_act(&x2cat.a, (size_t)N * H2 * W2 * x2cat.Cp, st));
    if (cfg.inference_only != 1) MIMO_TRY(alloc_act(&x2cat.da, (size_t)N * H2 * W2 * x2cat.Cp, st));
    x2cat.chmap.assign(x2cat.Cp, -1);
    for (int s = 0; s < S; ++s)
      for (int c = 0; c < 2 * f; ++c) x2cat.chmap[s * c2p + c] = s * 2 * f + c;
    for (int s = 0; s < S; ++s) {
      DoubleConv* dc;
      MIMO_TRY(make_dc(&dc, "encoder.down1s." + std::to_string(s) + ".conv.double_conv", enc_in[s]->out.chmap, f, 2 * f,
                       2 * f, H2, W2, cfg.encoder_dropout_rate, eoff(x2cat.a, (size_t)s * c2p), x2cat.Cp,
                       x2cat.da ? eoff(x2cat.da, (size_t)s * c2p) : nullptr, x2cat.Cp));
      MIMO_TRY(set_input(dc, IN_POOL, &enc_in[s]->out, nullptr, enc_in[s]->out.Cp, H2, W2));
      dc->out.parent = &x2cat;
      dc->out.parent_choff = s * c2p;
      down1.push_back(dc);
    }
    encoder_param_floats = param_floats;  // everything registered so far belongs to the S encoders
    // ---- core (model.py:190-243) ----
    const float pc = cfg.core_dropout_rate;
    MIMO_TRY(make_dc(&down2, "core.down2.conv.double_conv", x2cat.chmap, 2 * f * S, 4 * f * S, 4 * f * S, H3, W3, pc,
                     nullptr, 0, nullptr, 0));
    MIMO_TRY(set_input(down2, IN_POOL, &x2cat, nullptr, x2cat.Cp, H3, W3));
    MIMO_TRY(make_dc(&down3, "core.down3.conv.double_conv", down2->out.chmap, 4 * f * S, 8 * f * S, 8 * f * S, H4, W4, pc,
                     nullptr, 0, nullptr, 0));
    MIMO_TRY(set_input(down3, IN_POOL, &down2->out, nullptr, down2->out.Cp, H4, W4));
    MIMO_TRY(make_dc(&down4, "core.down4.conv.double_conv", down3->out.chmap, 8 * f * S, 8 * f * S, 8 * f * S, H5, W5, pc,
                     nullptr, 0, nullptr, 0));
    MIMO_TRY(set_input(down4, IN_POOL, &down3->out, nullptr, down3->out.Cp, H5, W5));
    {
      std::vector<int> m = cat_map(down3->out, down4->out);
      MIMO_TRY(make_dc(&up1, "core.up1.conv.double_conv", m, 16 * f * S, 8 * f * S, 4 * f * S, H4, W4, pc, nullptr, 0,
                       nullptr, 0));
      MIMO_TRY(set_input(up1, IN_UPCAT, &down3->out, &down4->out, (int)m.size(), H4, W4));
      rehome_skip(down3->out, up1, {{down3, 0}});
    }
    {
      std::vector<int> m = cat_map(down2->out, up1->out);
      MIMO_TRY(make_dc(&up2, "core.up2.conv.double_conv", m, 8 * f * S, 4 * f * S, 2 * f * S, H3, W3, pc, nullptr, 0,
                       nullptr, 0));
      MIMO_TRY(set_input(up2, IN_UPCAT, &down2->out, &up1->out, (int)m.size(), H3, W3));
      rehome_skip(down2->out, up2, {{down2, 0}});
    }
    {
      std::vector<int> m = cat_map(x2cat, up2->out);
      MIMO_TRY(make_dc(&up3, "core.up3.conv.double_conv", m, 4 * f * S, 2 * f * S, f * S, H2, W2, pc, nullptr, 0, nullptr,
                       0));
      MIMO_TRY(set_input(up3, IN_UPCAT, &x2cat, &up2->out, (int)m.size(), H2, W2));
      std::vector<std::pair<DoubleConv*, int>> pr;
      for (int s = 0; s < S; ++s) pr.push_back({down1[s], s * c2p});
      rehome_skip(x2cat, up3, pr);
    }
    // the outputs of the core's Up blocks are read only by the next block's bilinear up-sampling: it applies their
    // BatchNorm + ReLU itself and the activated tensor is not written in a training forward (elide_output)
    elide_output(up1);
    elide_output(up2);
    elide_output(up3);
    // MaxPool2d inputs are produced by the BatchNorm + ReLU pass of the tensor they pool (one pass less per Down block)
    {
      auto fuse = [this](DoubleConv* producer, DoubleConv* consumer, int choff) {
        producer->c2.pool_out = eoff(consumer->in_buf, choff);
        producer->c2.pool_ld = consumer->in_ld;
        consumer->pool_fused = true;
      };
      for (int s = 0; s < S; ++s) fuse(enc_in[s], down1[s], 0);
      for (int s = 0; s < S; ++s) fuse(down1[s], down2, s * c2p);
      fuse(down2, down3, 0);
      fuse(down3, down4, 0);
    }
    // ---- decoder (model.py:260-297) ----
    const int cin_dec = f * S + f;
    for (int s = 0; s < S; ++s) {
      std::vector<int> m = cat_map(enc_in[s]->out, up3->out);
      DoubleConv* dc;
      MIMO_TRY(make_dc(&dc, "decoder.up4s." + std::to_string(s) + ".conv.double_conv", m, cin_dec, cin_dec / 2, f, H1, W1,
                       cfg.decoder_dropout_rate, nullptr, 0, nullptr, 0));
      MIMO_TRY(set_input(dc, IN_UPCAT, &enc_in[s]->out, &up3->out, (int)m.size(), H1, W1));
      rehome_skip(enc_in[s]->out, dc, {{enc_in[s], 0}});
      // read by the 1x1 head (forward and backward) only; the element-wise final dropout would need the activated tensor
      if (cfg.final_dropout_rate <= 0.f) elide_output(dc);
      up4.push_back(dc);
    }
    for (int s = 0; s < S; ++s) {
      Head h;
      h.s = s;
      const std::string p = "decoder.outcs." + std::to_string(s) + ".conv";
      h.off_w = add_tensor(p + ".weight", {Co, f, 1, 1}, 0);
      h.off_b = add_tensor(p + ".bias", {Co}, 0);
      heads.push_back(h);
    }

    // ---- scratch ----
    const int fp = pad_channels(f);
    cap_partial = std::max(cap_partial, (size_t)kEwMaxBlocks * (Co * fp + Co));
    if (cfg.inference_only == 1) cap_act = cap_pad = 1;  // backward scratch: never touched
    if (cfg.inference_only) cap_slab = 1;               // weight-gradient slabs
    if (cfg.inference_only != 1) MIMO_TRY(dalloc(&s_zero, cap_cout));
    MIMO_TRY(alloc_act(&s_dz, cap_act, st));
    {
      const char* we = getenv("MIMO_WGRAD_STREAM");
      // default ON (round 2): the weight gradient of layer L runs on a side stream beside the BatchNorm-backward /
      // gather kernels of layer L-1 (bandwidth-bound: they co-reside with the persistent MFMA workgroup on a CU) and
      // queues behind the data gradient of layer L; dz goes round DzRing::kSlots buffers.  Measured +1.7 ... +4.7 %
      // images/s on three boxes (within noise on a fourth); results are bit-identical to the single-stream order.
      // With the profiler armed (bench.py's second pass) everything runs on the caller's stream.
      wg_async = !(we && atoi(we) == 0) && !cfg.inference_only;
      for (int i = 0; i < DzRing::kSlots; ++i) ring.dz[i] = s_dz;
      if (!cfg.inference_only)
        for (int i = 0; i < DzRing::kSlots; ++i) MIMO_TRY(dalloc(&ring.dzmax[i], kDzMaxSlots));
      if (any_mixed_dz && !cfg.inference_only) {  // (read by weight gradients only)
        MIMO_TRY(dalloc(&ring.dzs[0], cap_act));
        for (int i = 1; i < DzRing::kSlots; ++i) ring.dzs[i] = ring.dzs[0];
        if (wg_async)
          for (int i = 1; i < DzRing::kSlots; ++i) MIMO_TRY(dalloc(&ring.dzs[i], cap_act));
      }
      if (wg_async) {
        for (int i = 1; i < DzRing::kSlots; ++i) MIMO_TRY(alloc_act(&ring.dz[i], cap_act, st));
        // LOWEST stream priority — not for the scheduling (round 4 measured no effect of the priority on the step) but for the
        // hardware queue: the runtime deals streams of one priority class round-robin onto a handful of hardware queues
        // (4 by default), and a side stream that lands on the caller's queue is silently serialised behind it — seen in
        // round 6 in bench.py's one-rank RCCL route, where the process group's streams had taken the other queues: no
        // overlap at all, 5.8 instead of 4.4 ms per step at 4 images per GPU (profiles/r06/b4/queue_collision.txt).  The
        // priority classes draw from separate queue pools, and callers run on default-priority streams.
        {
          int least = 0, greatest = 0;
          MIMO_HIP_CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
          if (least != greatest)
            MIMO_HIP_CHECK(hipStreamCreateWithPriority(&ring.side, hipStreamNonBlocking, least));
          else
            MIMO_HIP_CHECK(hipStreamCreateWithFlags(&ring.side, hipStreamNonBlocking));
        }
        for (int i = 0; i < DzRing::kSlots; ++i)
          for (hipEvent_t* e : {&ring.ev_dz[i], &ring.ev_wg[i]}) MIMO_HIP_CHECK(hipEventCreateWithFlags(e, hipEventDisableTiming));
        MIMO_HIP_CHECK(hipEventCreateWithFlags(&ring.ev_join, hipEventDisableTiming));
        MIMO_HIP_CHECK(hipEventCreateWithFlags(&ev_stage, hipEventDisableTiming));
      }
    }
    MIMO_TRY(alloc_act(&s_dxpadA, cap_pad, st));
    MIMO_TRY(alloc_act(&s_dxpadB, cap_pad, st));
    MIMO_TRY(dalloc(&s_wslab, cap_slab));
    if (cap_kpart) MIMO_TRY(dalloc(&s_kpart, cap_kpart));
    MIMO_TRY(dalloc(&s_partial, cap_partial));
    if (fuse_bwd_src && !cfg.inference_only) MIMO_TRY(dalloc(&s_headpart, (size_t)kBnReduceMaxBlocks * (2 * pad_channels(f) + 2)));
    MIMO_TRY(dalloc(&s_sums, cap_sums));
    MIMO_TRY(dalloc(&s_losspart, (size_t)S * 512));
    MIMO_TRY(dalloc(&d_status, 1));
    // ---- weight repack job tables ----
    {
      std::vector<PackJob> jobs, dg;
      for (auto& dc : dcs)
        for (ConvBN* L : {&dc->c1, &dc->c2}) {
          // (fp16 forward images follow the layer's max |w|, L->wmax; the data gradient's keep the fixed 2^8)
          const ConvDir &fw = L->r.fwd, &dg_ = L->r.dgrad;
          jobs.push_back(pack::make_job(PACK_FWD, cfg.precision, fw.split, L->Cout, L->Cin, L->cin_p, L->cout_p, fw.rows, fw.wide, fw.pair,
                                        L->fwd_row_map, L->cin_map, fw.split ? L->wf16 : (void*)L->wf, L->wmax, L->off_w, L->off_b, L->bias_p));
          dg.push_back(pack::make_job(PACK_DGRAD, cfg.precision, dg_.split, L->Cout, L->Cin, L->cin_p, L->cout_p, dg_.rows, dg_.wide, dg_.pair,
                                      L->dg_row_map, L->dg_col_map, dg_.split ? L->wd16 : (void*)L->wd, nullptr, L->off_w));
          fill_launches(*L);
        }
      n_fwd_jobs = (int)jobs.size();
      if (cfg.inference_only != 1) jobs.insert(jobs.end(), dg.begin(), dg.end());
      n_all_jobs = (int)jobs.size();
      for (auto& j : jobs) pack_max_total = std::max(pack_max_total, j.total);
      MIMO_TRY(dalloc(&pack_jobs, jobs.size()));
      MIMO_HIP_CHECK(hipMemcpy(pack_jobs, jobs.data(), jobs.size() * sizeof(PackJob), hipMemcpyHostToDevice));
    }
    // hipGraph staging
    const char* ge = getenv("MIMO_HIP_GRAPH");
    graph_enabled = !(ge && atoi(ge) == 0);
    MIMO_TRY(dalloc(&g_x, (size_t)N * S * Ci * H * W));
    MIMO_TRY(dalloc(&g_out, (size_t)N * S * Co * H * W));
    MIMO_TRY(dalloc(&g_perm, (size_t)S * N));
    {
      // training-step graphs: opt-in (MIMO_TRAIN_GRAPH=1).  Built, bit-identical to eager launches, and measured NEUTRAL
      // (profiles/r06/train_graph.txt: 4.42 vs 4.42 ms per step at 4 images per GPU, 24.1 vs 23.9 at batch 32; the host spends
      // 0.76 ms in the hipGraphLaunch of the ~190-node backward graph — what the eager launches cost it), so the default
      // keeps the launches eager
      const char* te = getenv("MIMO_TRAIN_GRAPH");
      train_graph = graph_enabled && !cfg.inference_only && te && atoi(te) != 0;
      if (train_graph) {
        MIMO_TRY(dalloc(&g_label, (size_t)N * (Co / 2) * H * W));
        MIMO_TRY(dalloc(&g_lmask, (size_t)N * H * W));
        MIMO_TRY(dalloc(&g_lperm, (size_t)S * N));
        MIMO_TRY(dalloc(&g_dloss, (size_t)S));
      }
    }
    g_masks.resize(dcs.size());
    for (size_t i = 0; i < dcs.size(); ++i) MIMO_TRY(dalloc(&g_masks[i], (size_t)N * dcs[i]->c2.Cout));
    {
      if ((int)dcs.size() + 1 + S > FwdCall::kMaxSites) {
        set_error("too many dropout sites (%d) for the in-engine generator", (int)dcs.size() + 1 + S);
        return MIMO_ERR_INVALID;
      }
      std::vector<Dropout2dSite> sites(dcs.size());
      for (size_t i = 0; i < dcs.size(); ++i) {
        sites[i] = Dropout2dSite{g_masks[i], N * dcs[i]->c2.Cout, dcs[i]->drop_p};
        max_site_count = std::max(max_site_count, sites[i].count);
      }
      MIMO_TRY(dalloc(&d_sites, sites.size()));
      MIMO_HIP_CHECK(hipMemcpy(d_sites, sites.data(), sites.size() * sizeof(Dropout2dSite), hipMemcpyHostToDevice));
      elem_rng_on.assign(1 + S, 0);
    }
    MIMO_HIP_CHECK(hipStreamCreateWithFlags(&cap_stream, hipStreamNonBlocking));
    return MIMO_OK;
  }

  // ------------------------------------------------------------------ forward ------------
  // every layer's forward weight layout (+ bias copy) and, with_dgrad, the transposed data-gradient layout:
  // one launch over the job table
  int pack_all(bool with_dgrad, hipStream_t st) {
    // (fp16 forward images: the layers' max |w| first — the scale of an image follows it from |w| >= 128 up, w16_scale)
    if ((cfg.precision == MIMO_PREC_SPLIT16 || cfg.precision == MIMO_PREC_FP16_MIXED) && wmax_used > 0) {
      MIMO_HIP_CHECK(hipMemsetAsync(wmax_pool, 0, (size_t)wmax_used * sizeof(unsigned), st));
      MIMO_TRY(wabsmax_jobs_launch(pack_jobs, n_fwd_jobs, pack_max_total, params, st, d_status));
    }
    return pack_jobs_launch(pack_jobs, with_dgrad ? n_all_jobs : n_fwd_jobs, pack_max_total, params, st);
  }

  // elide: the activated tensor of this layer is not written in this call (its readers apply BatchNorm + ReLU to z)
  int convbn_forward(ConvBN& L, const FwdCall& call, const float* mask, bool elide, hipStream_t st) {
    const bool training = call.training;
    // inference: BN(eval) + ReLU (+ channel-dropout) in the conv epilogue — not for the fp32-kernel image convolution
    // of the 16-bit storage modes, whose output type differs from the activation type
    const bool fused = call.no_grad && !(mixed && !L.r.fwd.split);
    if (!training && call.need_derive)
      MIMO_TRY(bn_eval_prepare_launch(L.Cout, L.cout_p, params + L.off_gamma, params + L.off_beta, bnbuf + L.off_rm,
                                      bnbuf + L.off_rv, cfg.bn_eps, L.mean, L.invstd, L.scale, L.shift, st, d_status));
    // Training forward only.  (A forward without a graph folds BatchNorm + ReLU into every convolution's epilogue, and an
    // eval-mode forward WITH a graph — FGSM — keeps the separate pass, whose finiteness test feeds the numerics status word:
    // the activated tensors exist in both.  The weight gradient applies scale / shift to z either way: identical values.)
    const bool fin = L.fuse_in && training && !call.no_grad;
    ConvLaunch a = L.fwd;
    if (fin) {
      a.x = L.in_z;
      a.ldx = L.ld_in_z;
      a.in_scale = L.in_scale;
      a.in_shift = L.in_shift;
    }
    if (fused) {  // the activation and its type instead of z
      a.y = L.a;
      a.ldy = L.ld_a;
      a.ep_scale = L.scale;
      a.ep_shift = L.shift;
      a.ep_mask = mask;
      a.ep_mask_ld = L.Cout;
      a.status = d_status;
    }
    a.stats = training ? s_partial : nullptr;
    int rows = 0;
    const int64_t P = (int64_t)L.N * L.H * L.W;
    int pr = prof.begin(MIMO_PROF_CONV_FWD, st);
    if (L.r.fwd.split)  // (training forward: with the K split of conv3x3_ksplit where that pays — few tiles, a long K walk)
      MIMO_TRY(conv3x3_bf16x3_launch_k(a, fwd_mode(), &rows, st, (training && !fused) ? s_kpart : nullptr, cap_kpart));
    else if (L.r.thin)
      MIMO_TRY(conv3x3_thin_launch(a, L.Cin, &rows, st));
    else
      MIMO_TRY(conv3x3_launch(a, &rows, st));
    prof.end(pr, 18.0 * L.Cin * L.Cout * (double)P, 4.0 * (double)P * (L.Cin + L.Cout), st);
    if (training) {
      if (rows <= kColsumMaxRows) {
        MIMO_TRY(bn_fwd_stats_launch(s_partial, rows, L.r.fwd.rows, L.Cout, L.cout_p, P, params + L.off_gamma,
                                     params + L.off_beta, bnbuf + L.off_rm, bnbuf + L.off_rv, cfg.bn_momentum, cfg.bn_eps,
                                     L.mean, L.invstd, L.scale, L.shift, d_status, st));
      } else {
        int chunks = 0;
        MIMO_TRY(rowsum_launch(s_partial, rows, 2 * L.r.fwd.rows, s_sums, &chunks, st));
        MIMO_TRY(bn_fwd_finalize_launch(s_sums, chunks, L.r.fwd.rows, L.Cout, L.cout_p, P, params + L.off_gamma,
                                        params + L.off_beta, bnbuf + L.off_rm, bnbuf + L.off_rv, cfg.bn_momentum,
                                        cfg.bn_eps, L.mean, L.invstd, L.scale, L.shift, d_status, st));
      }
    }
    if (!fused && !elide) {
      pr = prof.begin(MIMO_PROF_BN_RELU_FWD, st);
      if (L.pool_out)
        MIMO_TRY(bn_relu_pool_fwd_launch(L.bn, mask, L.a, L.ld_a, L.pool_out, L.pool_ld, training ? nullptr : d_status, st));
      else
        MIMO_TRY(bn_relu_fwd_launch(L.bn, mask, L.a, L.ld_a, training ? nullptr : d_status, st));
      prof.end(pr, 0.0, (L.pool_out ? 9.0 : 8.0) * (double)P * L.cout_p, st);
    }
    return MIMO_OK;
  }

  // Output activation of an Up block read through BatchNorm + ReLU by its consumers (Act::z): split16 training plans, no
  // Dropout2d on the block (its multipliers act on the activated tensor), MIMO_FUSE_BN_IN != 0.  The decoders' blocks
  // additionally need the element-wise final dropout off (checked where they are built).
  void elide_output(DoubleConv* dc) {
    if (!fuse_bn_in || cfg.precision != MIMO_PREC_SPLIT16 || cfg.inference_only || dc->drop_p > 0.f || dc->c2.pool_out ||
        dc->c2.r.dtz != ST_F32)
      return;
    dc->c2.act_elided = true;
    dc->out.z = dc->c2.z;
    dc->out.z_ld = dc->c2.cout_p;
    dc->out.z_scale = dc->c2.scale;
    dc->out.z_shift = dc->c2.shift;
  }

  // the readers of this block's output go through z in this call (Act::z_live); dc->mask must be this call's
  bool z_live_rule(const DoubleConv* dc, const FwdCall& call, bool elem_mask_on_output) const {
    return dc->c2.act_elided && dc->out.z && call.training && !call.no_grad && !dc->mask && !elem_mask_on_output;
  }

  int dc_forward(DoubleConv* dc, const FwdCall& call, hipStream_t st) {
    const int h = dc->c1.H, w = dc->c1.W;
    const int blk = prof.begin(Profiler::kTierBase + 2 * tier_of(h), st);
    if (dc->kind == IN_POOL) {
      Act* s = dc->src0;
      if (!(dc->pool_fused && !call.no_grad))  // else: already written by the producers' BatchNorm + ReLU pass
        MIMO_TRY(maxpool_fwd_launch(s->a, this->st, s->ld, N, s->H, s->W, s->Cp, dc->in_buf, dc->in_ld, st));
    } else if (dc->kind == IN_UPCAT) {
      Act *sk = dc->src0, *lo = dc->src1;
      const int pr = prof.begin(MIMO_PROF_UPCAT_FWD, st);
      const bool lz = lo->z_live;  // the low-resolution tensor through its BatchNorm + ReLU
      MIMO_TRY(upcat_fwd_launch(nullptr, this->st, sk->ld, sk->Cp, lz ? lo->z : lo->a,
                                lz ? lo->z_ld : lo->ld, lo->Cp, N, h, w, lo->H, lo->W, dc->in_buf, st, lz ? lo->z_scale : nullptr,
                                lz ? lo->z_shift : nullptr));
      // writes the up-sampled channels at (h, w), reads the low-resolution tensor once
      prof.end(pr, 0.0, 4.0 * lo->Cp * ((double)N * h * w + (double)N * lo->H * lo->W), st);
    }

    MIMO_TRY(convbn_forward(dc->c1, call, nullptr, dc->c1.act_elided && call.training, st));
    MIMO_TRY(convbn_forward(dc->c2, call, dc->mask, dc->out.z_live, st));
    prof.end(blk, 0.0, 0.0, st);
    return MIMO_OK;
  }

  int check_forward(const mimo_forward_args* args) const {
    if (!params || !bnbuf) {
      set_error("mimo_forward: parameters not bound (mimo_plan_bind)");
      return MIMO_ERR_STATE;
    }
    if (!args || !args->x || !args->out) {
      set_error("mimo_forward: null argument");
      return MIMO_ERR_INVALID;
    }
    if (cfg.inference_only == 1 && (args->training || !args->no_grad)) {
      set_error("mimo_forward: inference-only plan (mimo_config.inference_only) needs training = 0 and no_grad = 1");
      return MIMO_ERR_STATE;
    }
    if (cfg.inference_only == 2 && args->training) {
      set_error("mimo_forward: input-gradient-only plan (mimo_config.inference_only = 2) needs training = 0");
      return MIMO_ERR_STATE;
    }
    return MIMO_OK;
  }

  // the call as the issuing functions see it; *active: the Dropout2d sites whose multipliers the engine draws (into g_masks)
  FwdCall make_call(const mimo_forward_args& a, uint64_t* active) const {
    FwdCall c;
    const int ndc = (int)dcs.size();
    c.x = a.x;
    c.stride_n = a.stride_n;
    c.stride_s = a.stride_s;
    c.perm = a.perm;
    c.out = a.out;
    c.rows = a.x_rows > 0 ? a.x_rows : N;
    const int64_t img = (int64_t)Ci * H * W;
    c.x5 = a.stride_s == img && a.stride_n == (int64_t)S * img;
    c.x4 = a.stride_s == 0 && a.stride_n == img;
    *active = 0;
    for (int i = 0; i < ndc; ++i) {
      c.masks[i] = a.drop_masks ? a.drop_masks[i] : nullptr;
      if (a.rng_sites && a.rng_sites[i] && dcs[i]->drop_p > 0.f) {
        *active |= 1ull << i;
        c.masks[i] = g_masks[i];
      }
    }
    c.rng_seed = a.rng_seed;
    c.rng_offset = a.rng_offset;
    c.elem_dropout = a.elem_masks != nullptr;
    for (int j = 0; j <= S; ++j) {
      c.elem_masks[j] = a.elem_masks ? a.elem_masks[j] : nullptr;
      c.elem_rng_on[j] = a.rng_sites && a.rng_sites[ndc + j] && elem_rate(j) > 0.f && !c.elem_masks[j];
      c.elem_dropout |= c.elem_rng_on[j];
    }
    // what has to be (re)derived from the parameters in this call, and whether anything is kept for a backward
    c.training = a.training != 0;
    c.no_grad = !c.training && a.no_grad != 0;
    c.need_derive = c.training || a.param_version == 0 || a.param_version != derived_version;
    // (-1 after a training forward: the optimiser step invalidates the packed weights)
    c.version_after = c.training ? -1 : (a.param_version != 0 ? a.param_version : -1);
    return c;
  }

  // the same call on the plan's staging copies: what a captured forward reads and writes
  FwdCall staged_call(const FwdCall& call) const {
    FwdCall g = call;
    g.x = g_x;
    g.perm = call.perm ? g_perm : nullptr;
    g.out = g_out;
    for (size_t i = 0; i < dcs.size(); ++i) g.masks[i] = call.masks[i] ? g_masks[i] : nullptr;
    return g;
  }

  // the caller's x / perm / Dropout2d multipliers into the staging copies
  int stage_inputs(const FwdCall& call, hipStream_t st) {
    MIMO_HIP_CHECK(hipMemcpyAsync(g_x, call.x, (size_t)call.rows * (call.x5 ? S : 1) * Ci * H * W * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (call.perm)
      MIMO_HIP_CHECK(hipMemcpyAsync(g_perm, call.perm, (size_t)S * N * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    for (size_t i = 0; i < dcs.size(); ++i)
      if (call.masks[i] && call.masks[i] != g_masks[i])  // (an in-engine site was drawn straight into the staging buffer)
        MIMO_HIP_CHECK(hipMemcpyAsync(g_masks[i], call.masks[i], (size_t)N * dcs[i]->c2.Cout * sizeof(float),
                                      hipMemcpyDeviceToDevice, st));
    return MIMO_OK;
  }

  // In front of issuing or replaying a forward: what of the call's state lives on the blocks — this call's Dropout2d
  // multipliers and which activated tensors are read through z (every input of that rule is known before the first launch).
  void prepare_forward(const FwdCall& call) {
    for (size_t i = 0; i < dcs.size(); ++i) {
      dcs[i]->mask = call.masks[i];
      dcs[i]->out.z_live = z_live_rule(dcs[i].get(), call, false);
    }
    // (an element-wise final dropout on a block whose output is elided by construction: this call materialises it)
    for (int s = 0; s < S; ++s) up4[s]->out.z_live = z_live_rule(up4[s], call, call.elem_on(1 + s));
  }

  // Behind a forward that was issued or replayed: what the loss and the backward read later.  `call` carries the pointers they
  // are to see — the caller's after an eager forward and after an eval-mode replay, the staged ones after a training replay
  // (graphed: a backward graph must not see the caller's pointers).
  void record_forward(const FwdCall& call, bool graphed, const int64_t* perm_arg) {
    out = call.out;
    fwd_done = true;
    fwd_training = call.training;
    fwd_no_grad = call.no_grad;
    had_perm = call.perm != nullptr;
    loss_done = false;
    elem_masks.assign(call.elem_masks, call.elem_masks + 1 + S);
    elem_rng_on.assign(call.elem_rng_on, call.elem_rng_on + 1 + S);
    rng_seed = call.rng_seed;
    rng_offset = call.rng_offset;
    fwd_graphed = graphed;
    last_x_rows = call.rows;
    last_perm_arg = graphed ? perm_arg : nullptr;
    derived_version = call.version_after;
  }

  int forward(const mimo_forward_args* args, hipStream_t st) {
    MIMO_TRY(check_forward(args));
    // ---- in-engine dropout: draw the Dropout2d multipliers of the flagged sites, note the element-wise ones ----
    uint64_t active = 0;
    const FwdCall call = make_call(*args, &active);
    MIMO_TRY(dropout2d_masks_launch(d_sites, (int)dcs.size(), max_site_count, active, call.rng_seed, call.rng_offset, st));
    fwd_graphed = loss_staged = false;  // whatever the previous forward staged for a backward graph ends here, also if this call fails
    // eval mode replays a graph while the packed weights stand (need_derive: the repack is not part of that graph); a
    // training forward always repacks — inside its graph
    const bool graphable = graph_enabled && !prof.on && (call.x5 || call.x4) && !call.elem_dropout && call.rows <= N &&
                           (call.training ? train_graph : !call.need_derive);
    uint64_t key = 1 | (call.x5 ? 2 : 0) | (call.perm ? 4 : 0) | (call.no_grad ? 8 : 0) | (call.training ? 16 : 0);
    for (size_t i = 0; i < dcs.size(); ++i)
      if (call.masks[i]) key |= 1ull << (8 + i);
    sched::GraphReplayPolicy& replay = call.training ? tg_fwd_replay : eval_replay;
    const auto route = graphable ? replay.decide(key) : sched::GraphReplayPolicy::Eager;
    if (route == sched::GraphReplayPolicy::Eager) {
      prepare_forward(call);
      if (const int rc = forward_impl(call, st)) {
        derived_version = -1;
        return rc;
      }
      record_forward(call, false, nullptr);
      return MIMO_OK;
    }
    // ---- stage the caller's tensors, (re)capture if the call shape changed, replay ----
    const FwdCall staged = staged_call(call);
    hipGraphExec_t* exec = call.training ? &tg_fwd : &graph_exec;
    int rc = stage_inputs(call, st);
    if (rc == MIMO_OK && route == sched::GraphReplayPolicy::Capture) {
      destroy_exec(exec);
      prepare_forward(staged);  // (the issuing functions read the blocks' masks and z_live)
      rc = capture([&](hipStream_t cs) { return forward_impl(staged, cs); }, exec);
    }
    if (rc != MIMO_OK) {
      if (route == sched::GraphReplayPolicy::Capture) replay.capture_failed();
      return rc;
    }
    // the loss and the backward after a training replay stay on the staged tensors; an eval-mode forward writes every
    // activated tensor, and its backward (FGSM) reads the caller's masks and logits
    const FwdCall& left = call.training ? staged : call;
    prepare_forward(left);
    MIMO_HIP_CHECK(hipGraphLaunch(*exec, st));
    MIMO_HIP_CHECK(hipMemcpyAsync(call.out, g_out, (size_t)N * S * Co * H * W * sizeof(float), hipMemcpyDeviceToDevice, st));
    record_forward(left, call.training, call.perm);
    return MIMO_OK;
  }

  // run `body` under stream capture on cap_stream and instantiate the resulting graph
  template <typename F>
  int capture(F body, hipGraphExec_t* exec) {
    MIMO_HIP_CHECK(hipStreamBeginCapture(cap_stream, hipStreamCaptureModeThreadLocal));
    capturing = true;
    const int rc = body(cap_stream);
    capturing = false;
    hipGraph_t graph = nullptr;
    const hipError_t ce = hipStreamEndCapture(cap_stream, &graph);
    if (rc != MIMO_OK) {
      if (graph) (void)hipGraphDestroy(graph);
      return rc;
    }
    MIMO_HIP_CHECK(ce);
    const hipError_t ie = hipGraphInstantiate(exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    MIMO_HIP_CHECK(ie);
    return MIMO_OK;
  }

  // issues one forward on `st` (eagerly or under capture); prepare_forward(call) has run
  int forward_impl(const FwdCall& call, hipStream_t st) {
    if (call.need_derive) MIMO_TRY(pack_all(call.training, st));
    for (int s = 0; s < S; ++s)
      MIMO_TRY(pack_input_launch(call.x, call.stride_n, call.stride_s, call.perm, s, N, Ci, H, W, enc_in[s]->in_buf,
                                 Ci_p, st));
    for (int s = 0; s < S; ++s) {  // chain by chain
      MIMO_TRY(dc_forward(enc_in[s], call, st));
      MIMO_TRY(dc_forward(down1[s], call, st));
    }
    MIMO_TRY(dc_forward(down2, call, st));
    MIMO_TRY(dc_forward(down3, call, st));
    MIMO_TRY(dc_forward(down4, call, st));
    // center_dropout: in place on down4's output, whose only reader is up1's upsample (the BN/ReLU
    // backward recomputes its mask from z, not from a)
    if (call.elem_on(0)) {
      const ElemRng g = elem_rng(0, call.rng_seed, call.rng_offset);
      MIMO_TRY(elem_mask_mul_launch(down4->out.a, this->st, down4->out.ld, call.elem_masks[0], N, down4->out.C, down4->out.Cp,
                                    down4->out.H * down4->out.W, st, call.elem_masks[0] ? nullptr : &g));
    }
    MIMO_TRY(dc_forward(up1, call, st));
    MIMO_TRY(dc_forward(up2, call, st));
    MIMO_TRY(dc_forward(up3, call, st));
    for (int s = 0; s < S; ++s) {
      MIMO_TRY(dc_forward(up4[s], call, st));
      const Act& o = up4[s]->out;
      // final_dropouts[s]: in place, the head (forward and weight gradient) is the only reader
      if (call.elem_on(1 + s)) {
        const ElemRng g = elem_rng(1 + s, call.rng_seed, call.rng_offset);
        MIMO_TRY(elem_mask_mul_launch(o.a, this->st, o.ld, call.elem_masks[1 + s], N, o.C, o.Cp, H * W, st,
                                      call.elem_masks[1 + s] ? nullptr : &g));
      }
      const int blk = prof.begin(Profiler::kTierBase, st);
      const int pr = prof.begin(MIMO_PROF_HEAD_FWD, st);
      const bool oz = o.z_live;
      MIMO_TRY(head_fwd_launch(oz ? o.z : o.a, this->st, oz ? o.z_ld : o.ld, params + heads[s].off_w, params + heads[s].off_b, f, Co,
                               N, S, s, H * W, call.out, st, d_status, oz ? o.z_scale : nullptr, oz ? o.z_shift : nullptr));
      prof.end(pr, 0.0, 4.0 * (double)N * H * W * (pad_channels(f) + Co), st);
      prof.end(blk, 0.0, 0.0, st);
    }
    return MIMO_OK;
  }

  int loss_forward(const float* label_, const float* mask_, const int64_t* perm_, float* loss_out, hipStream_t st) {
    if (!fwd_done) {
      set_error("mimo_loss_forward: call mimo_forward first");
      return MIMO_ERR_STATE;
    }
    if (!label_ || !loss_out) {
      set_error("mimo_loss_forward: null argument");
      return MIMO_ERR_INVALID;
    }
    loss_staged = false;
    if (fwd_graphed && train_graph && last_x_rows >= 1 && last_x_rows <= N) {
      // a backward graph reads label / mask / perm: plan-owned copies (the batch's tensors have last_x_rows rows)
      const size_t hw = (size_t)H * W;
      MIMO_HIP_CHECK(hipMemcpyAsync(g_label, label_, (size_t)last_x_rows * (Co / 2) * hw * sizeof(float), hipMemcpyDeviceToDevice, st));
      label_ = g_label;
      if (mask_) {
        MIMO_HIP_CHECK(hipMemcpyAsync(g_lmask, mask_, (size_t)last_x_rows * hw * sizeof(float), hipMemcpyDeviceToDevice, st));
        mask_ = g_lmask;
      }
      if (perm_ && perm_ == last_perm_arg) {
        perm_ = g_perm;  // the forward staged this very tensor
      } else if (perm_) {
        MIMO_HIP_CHECK(hipMemcpyAsync(g_lperm, perm_, (size_t)S * N * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
        perm_ = g_lperm;
      }
      loss_staged = true;
    }
    int blocks = 0;
    MIMO_TRY(loss_fwd_launch(out, label_, mask_, perm_, N, S, Co, H * W, cfg.loss_kind, cfg.eps_min, cfg.eps_max,
                             s_losspart, &blocks, st));
    MIMO_TRY(loss_finalize_launch(s_losspart, S, blocks, (double)N * (Co / 2) * H * W, loss_out, st));
    label = label_;
    lmask = mask_;
    lperm = perm_;
    loss_done = true;
    return MIMO_OK;
  }

  // ------------------------------------------------------------------ backward -----------
  // gradient arriving at an activation: first writer assigns, later writers accumulate
  static int acc_flag(Act* t) { return t->grad_writes++ > 0 ? 1 : 0; }

  // data gradient of layer L on the reflect-padded domain: dxpad_out [N,H+2,W+2,cin_p] from dz
  int dgrad_conv(ConvBN& L, const float* dz, float* dxpad_out, hipStream_t st) {
    const int64_t P = (int64_t)L.N * L.H * L.W;
    ConvLaunch a = L.dgrad;
    a.x = dz;
    a.y = dxpad_out;
    int pr = prof.begin(MIMO_PROF_CONV_DGRAD, st);
    if (L.r.dgrad.split)
      MIMO_TRY(conv3x3_bf16x3_launch_k(a, dgrad_mode(), nullptr, st, s_kpart, cap_kpart));
    else
      MIMO_TRY(conv3x3_launch(a, nullptr, st));
    prof.end(pr, 18.0 * L.Cin * L.Cout * (double)P, 4.0 * (double)P * (L.Cin + L.Cout), st);
    return MIMO_OK;
  }

  // algorithmic bytes of the gradient source per pixel and channel (z and dz are counted by the passes themselves): the pooled
  // gradient is a quarter of the image, the head's logits / labels a few floats per pixel
  static double src_bytes(const GradSrc& src) {
    return src.kind == GS_POOL ? (1.0 + (src.skip ? 4.0 : 0.0)) : src.kind == GS_HEAD ? 0.5 : 4.0;
  }

  // pass 2 of the BatchNorm + ReLU backward of layer L: dz = scale * (dy - c1 - xhat * c2) into `dz`
  // partial != nullptr: + partial rows of sum dz; absmax / done: bn_bwd_apply_launch
  int bn_apply(ConvBN& L, const GradSrc& src, const float* mask, const float* c1, const float* c2, float* dz, bool split_out,
               float* partial, int* rows, hipStream_t st, float* absmax = nullptr, int* absmax_n = nullptr, hipEvent_t done = nullptr) {
    const int64_t P = (int64_t)L.N * L.H * L.W;
    const int pr = prof.begin(MIMO_PROF_BN_BWD_APPLY, st);
    MIMO_TRY(bn_bwd_apply_launch(L.bn, src, mask, BnBwdApplyOut{c1, c2, dz, split_out ? 1 : 0, partial, rows, absmax, absmax_n, done}, st));
    prof.end(pr, 0.0, (8.0 + src_bytes(src)) * (double)P * L.cout_p, st);
    return MIMO_OK;
  }

  // mimo_input_gradient's form of convbn_backward: after an eval-mode forward BatchNorm is the fixed affine map of its running
  // statistics, so its backward is dz = scale * relu'(.) * dy — bn_bwd_apply_kernel with c1 = c2 = 0 (the constant zero vector
  // s_zero; mimo_backward's eval branch reaches the same zeros through the reduction pass and bn_bwd_stats_kernel, and the same
  // bits).  No reduction, no column sums, no max |dz| slots, no event, nothing written outside the plan's scratch.
  int convbn_input_grad(ConvBN& L, const GradSrc& src, const float* mask, float* dxpad_out, hipStream_t st) {
    float* dz = ring.dz[0];
    int rows = 0;
    MIMO_TRY(bn_apply(L, src, mask, s_zero, s_zero, dz, L.r.dgrad.split && !mixed, nullptr, &rows, st));
    return dgrad_conv(L, dz, dxpad_out, st);
  }

  // BatchNorm + ReLU backward of layer L (`src`: where the gradient arriving at L's activation comes from, GradSrc,
  // elementwise.h): BatchNorm parameter gradients, dz into slot `s` of the ring — released to the weight gradient behind its
  // last writer — and the convolution's bias gradient.  training: the forward used batch statistics.
  // thin_wg: the weight gradient reads dz as fp32 and nothing else reads it.
  int bn_backward(ConvBN& L, const GradSrc& src, const float* mask, DzRing::Slot& s, bool training, bool thin_wg, hipStream_t st) {
    int rows = 0;
    const int64_t P = (int64_t)L.N * L.H * L.W;
    const int pr = prof.begin(MIMO_PROF_BN_BWD_REDUCE, st);
    MIMO_TRY(bnrelu_bwd_reduce_launch(L.bn, src, mask, s_partial, &rows, st));
    prof.end(pr, 0.0, (4.0 + src_bytes(src)) * (double)P * L.cout_p, st);
    if (src.kind == GS_HEAD) head_rows = rows;
    MIMO_TRY(bn_bwd_stats_launch(s_partial, rows, L.Cout, L.cout_p, P, training ? 1 : 0, L.c1, L.c2, grads + L.off_gamma,
                                 grads + L.off_beta, training ? grads + L.off_b : nullptr, d_status, st));
    MIMO_TRY(ring.wait_free(s, st));
    float* dz = ring.dz[s.b];
    // dz storage: bf16 hi|lo pairs when the data-gradient kernel is the bf16-pair one (then the weight
    // gradient is too); fp32 otherwise, with a split copy for a bf16-pair weight gradient
    const bool needs_split_copy = L.r.wg_split && !L.r.dgrad.split && !thin_wg;
    if (L.r.wg_np2 && !thin_wg) s.absmax = ring.dzmax[s.b];  // (travels with the dz buffer it describes: same slot, same events)
    MIMO_TRY(bn_apply(L, src, mask, L.c1, L.c2, dz, L.r.dgrad.split && !mixed && !thin_wg, training ? nullptr : s_partial, &rows, st,
                      s.absmax, &s.absmax_n, ring.dz_event_on_launch(s, capturing, needs_split_copy)));
    s.dz_wg = dz;
    if (needs_split_copy) {
      MIMO_TRY(split_pairs_launch(dz, ring.dzs[s.b], P, L.cout_p, st));
      s.dz_wg = ring.dzs[s.b];
    }
    MIMO_TRY(ring.dz_written(s, st));
    // conv bias gradient: exactly zero in front of a training-mode BatchNorm (written by bn_bwd_stats above);
    // a real column sum of dz only after an eval-mode forward (running statistics: dz = scale * dy)
    if (!training) MIMO_TRY(colsum_vec_launch(s_partial, rows, L.cout_p, L.Cout, grads + L.off_b, st));
    return MIMO_OK;
  }

  // weight gradient of layer L and its reduction on `ws`; release != nullptr: recorded when the reduction completes
  int wgrad_issue(ConvBN& L, const DzRing::Slot& o, bool thin_wg, hipStream_t ws, hipEvent_t release) {
    const int64_t P = (int64_t)L.N * L.H * L.W;
    WgradLaunch wg = L.wgrad;
    wg.dz = o.dz_wg;
    if (o.absmax) {  // two fp16 MFMAs per product (wgrad_split.hip NP == 2; bn_backward hands the slots out where r.wg_np2)
      wg.np = 2;
      wg.dz_absmax = o.absmax;
      wg.dz_absmax_n = o.absmax_n;
    }
    if (wg_delay_us > 0) MIMO_TRY(debug_delay_launch(wg_delay_us, ws));  // test hook: a late consumer
    const int pr = prof.begin(MIMO_PROF_CONV_WGRAD, ws);
    if (thin_wg)  // (dz as fp32, straight from the BatchNorm backward)
      MIMO_TRY(wgrad_thin_launch(L.in, L.ld_in, o.dz_wg, L.cout_p, L.N, L.H, L.W, L.Cin, L.Cout, L.cout_p, s_wslab, grads + L.off_w, ws));
    else if (L.r.wg_split)
      MIMO_TRY(wgrad_split_launch(wg, ws));
    else
      MIMO_TRY(wgrad_launch(wg, ws));
    prof.end(pr, 18.0 * L.Cin * L.Cout * (double)P, 4.0 * (double)P * (L.Cin + L.Cout), ws);
    if (!thin_wg)  // (the plain-FMA kernel's launch reduces its own partials)
      MIMO_TRY(wgrad_reduce_launch(s_wslab, wg.splits, wg.cin_pad, wg.cout_pad, L.cin_map, L.cin_p, L.Cin, L.Cout,
                                   grads + L.off_w, ws, wg.dz_absmax, wg.dz_absmax_n, release));
    return MIMO_OK;
  }

  int convbn_backward(ConvBN& L, const GradSrc& src, const float* mask, bool need_dgrad, float* dxpad_out, const BwdCall& call,
                      hipStream_t st) {
    if (call.ig) return need_dgrad ? convbn_input_grad(L, src, mask, dxpad_out, st) : MIMO_OK;
    // the image convolution's weight gradient on the plain-FMA kernel reads dz as fp32 (no data gradient wanted: nothing
    // else reads this dz)
    const bool thin_wg = L.r.wg_thin && !need_dgrad && wgrad_thin_ok(L.Cin, L.cout_p, L.N, L.H, L.W);
    // (with the profiler armed everything runs on the caller's stream: per-kernel times, not overlapped times)
    DzRing::Slot s = ring.acquire(wg_async && !prof.on);
    MIMO_TRY(bn_backward(L, src, mask, s, fwd_training, thin_wg, st));
    if (need_dgrad) MIMO_TRY(dgrad_conv(L, ring.dz[s.b], dxpad_out, st));
    hipStream_t ws = st;
    MIMO_TRY(ring.reader_stream(s, st, &ws));
    const hipEvent_t release = ring.release_on_launch(s, capturing, thin_wg);
    MIMO_TRY(wgrad_issue(L, s, thin_wg, ws, release));
    return ring.released(s, release != nullptr);
  }

  int dc_backward(DoubleConv* dc, bool need_input_grad, const BwdCall& call, hipStream_t st, const GradSrc* head_src = nullptr) {
    const int blk = prof.begin(Profiler::kTierBase + 2 * tier_of(dc->c1.H) + 1, st);
    const int rc = dc_backward_impl(dc, need_input_grad, call, st, head_src);
    prof.end(blk, 0.0, 0.0, st);
    return rc;
  }

  int dc_backward_impl(DoubleConv* dc, bool need_input_grad, const BwdCall& call, hipStream_t st, const GradSrc* head_src) {
    GradSrc src = GradSrc::plain(dc->out.da, dc->out.ldda);
    {
      const Act* root = dc->out.parent ? dc->out.parent : &dc->out;
      if (head_src) {
        src = *head_src;
      } else if (root->poolgrad) {  // pooled by a Down block that left its gradient in place (below)
        src.kind = GS_POOL;
        src.dxpad = root->poolgrad;
        src.ldp = root->poolgrad_ld;
        src.skip = root->skipgrad;
        src.ldsk = root->skipgrad_ld;
        src.choff = src.skoff = dc->out.parent ? dc->out.parent_choff : 0;
      }
    }
    MIMO_TRY(convbn_backward(dc->c2, src, dc->mask, true, s_dxpadA, call, st));
    float* dxB = dc->dxpad_own ? dc->dxpad_own : s_dxpadB;
    MIMO_TRY(convbn_backward(dc->c1, GradSrc::fold(s_dxpadA, dc->c1.cout_p), nullptr, need_input_grad, dxB, call, st));
    if (!need_input_grad) return MIMO_OK;
    const int h = dc->c1.H, w = dc->c1.W, ldp = dc->c1.cin_p;
    if (dc->kind == IN_POOL && fuse_bwd_pool && dc->dxpad_own && dc->src0->grad_writes == 0) {
      // nobody has written the pooled tensor's gradient buffer (its skip gradient, if any, waits in the Up block's own
      // buffer): the producers' BatchNorm backward reads pool route + skip fold straight from the two padded-domain buffers
      Act* s = dc->src0;
      s->poolgrad = dxB;
      s->poolgrad_ld = ldp;
    } else if (dc->kind == IN_POOL) {
      Act* s = dc->src0;
      const int pr = prof.begin(MIMO_PROF_POOL_BWD, st);
      const bool acc = acc_flag(s) != 0;
      MIMO_TRY(pool_bwd_launch(dxB, this->st, ldp, 0, s->a, s->ld, s->da, s->ldda, N, s->H, s->W, s->Cp, acc ? 1 : 0, st, s->skipgrad,
                               s->skipgrad_ld));
      // reads the pooled gradient (1/4), the activation, [the skip gradient], [the old gradient]; writes the gradient
      prof.end(pr, 0.0, 4.0 * s->Cp * (double)N * s->H * s->W * (2.25 + (s->skipgrad ? 1.0 : 0.0) + (acc ? 1.0 : 0.0)), st);
      s->skipgrad = nullptr;
    } else if (dc->kind == IN_UPCAT) {
      Act *sk = dc->src0, *lo = dc->src1;
      // the skip slice stays where the data gradient wrote it (dxpad_own); the pool backward of sk folds it in
      sk->skipgrad = dxB;
      sk->skipgrad_ld = ldp;
      const int pr = prof.begin(MIMO_PROF_UP_BWD, st);
      MIMO_TRY(up_bwd_launch(dxB, this->st, ldp, sk->Cp, lo->da, lo->ldda, N, h, w, lo->H, lo->W, lo->Cp, acc_flag(lo), st));
      // reads the up-sampled slice of the padded-domain gradient once, writes the low-resolution gradient
      prof.end(pr, 0.0, 4.0 * lo->Cp * ((double)N * (h + 2) * (w + 2) + (double)N * lo->H * lo->W), st);
    }
    return MIMO_OK;
  }

  // The backward in kBwdStages stages, in execution order; each stage's parameters are one contiguous range of the
  // flat gradient buffer (laid out encoder | core down2..up3 | decoder | heads), final when the stage returns, so a
  // data-parallel caller can start that range's all-reduce while the later stages run:
  //   0 heads + decoders (up4)   1 up3   2 up2   3 up1   4 down4   5 down3   6 down2   7 encoders (+ dx)
  static constexpr int kBwdStages = 8;
  void stage_range(int stage, int64_t* b, int64_t* e) const {
    DoubleConv* core[6] = {up3, up2, up1, down4, down3, down2};
    if (stage == 0) {
      *b = up4[0]->p_begin;
      *e = param_floats;
    } else if (stage == kBwdStages - 1) {
      *b = 0;
      *e = encoder_param_floats;
    } else {
      *b = core[stage - 1]->p_begin;
      *e = core[stage - 1]->p_end;
    }
  }

  // ready != nullptr (mimo_backward_stage_async): the stage's gradient range need only be final on the stream returned in
  // *ready — the side stream when the weight gradients run there (it first waits for the caller's stream: BatchNorm and head
  // gradients are written there) — and the caller's stream is NOT made to wait for the side stream: a data-parallel caller
  // issues the range's collective on *ready, and the main stream goes straight on with the next stage.  The last stage joins.
  int backward(const float* dout, const float* dloss, float* dx, int stage_first, int stage_last, hipStream_t st,
               hipStream_t* ready = nullptr) {
    if (ready) *ready = st;
    MIMO_TRY(check_backward(dout, dloss, dx, stage_first, stage_last));
    const bool whole = stage_first == 0 && stage_last == kBwdStages - 1;
    const bool graph_shaped = !dout && !dx && (whole || stage_first == stage_last);  // what a backward graph can stand for
    if (stage_first == 0) MIMO_TRY(backward_graphs(dloss, whole, graph_shaped && dloss && !ready, st));
    if (tg_bwd_live) return backward_replay(stage_first, stage_last, whole, graph_shaped, st);
    return backward_eager(BwdCall{dout, dloss, dx}, stage_first, stage_last, ready, st);
  }

  int check_backward(const float* dout, const float* dloss, const float* dx, int stage_first, int stage_last) const {
    if (!fwd_done) {
      set_error("mimo_backward: call mimo_forward first");
      return MIMO_ERR_STATE;
    }
    if (cfg.inference_only == 2) {
      set_error("mimo_backward: input-gradient-only plan (mimo_config.inference_only = 2): only mimo_input_gradient runs on it");
      return MIMO_ERR_STATE;
    }
    if (!grads) {
      set_error("mimo_backward: gradient buffer not bound");
      return MIMO_ERR_STATE;
    }
    if (fwd_no_grad) {
      set_error("mimo_backward: the last forward ran with no_grad (inference epilogue, nothing saved)");
      return MIMO_ERR_STATE;
    }
    if (!dout && !dloss) {
      set_error("mimo_backward: need dout and/or dloss");
      return MIMO_ERR_INVALID;
    }
    if (dloss && !loss_done) {
      set_error("mimo_backward: dloss given but mimo_loss_forward was not called");
      return MIMO_ERR_STATE;
    }
    if (dx && had_perm) {
      set_error("mimo_backward: dx requires a forward without perm");
      return MIMO_ERR_INVALID;
    }
    if (stage_first < 0 || stage_last >= kBwdStages || stage_first > stage_last) {
      set_error("mimo_backward: bad stage range %d..%d", stage_first, stage_last);
      return MIMO_ERR_INVALID;
    }
    if (stage_first != 0 && stage_first != bwd_next_stage) {
      set_error("mimo_backward: stage %d requested, stage %d is next", stage_first, bwd_next_stage);
      return MIMO_ERR_STATE;
    }
    return MIMO_OK;
  }

  // Stage 0 of a backward: decides whether this backward replays training-step graphs (tg_bwd_live), captures them on the
  // second sighting of the call shape — the whole backward as one graph or each of the eight stages as its own — and stages dloss.
  // shape_ok: the call is one a graph can stand for (dloss only, whole or a single stage, not the asynchronous stages —
  // `ready` — which are eager launches: a per-stage graph has to close its fork to the side stream before it ends, which is
  // the join that route exists to avoid).
  int backward_graphs(const float* dloss, bool whole, bool shape_ok, hipStream_t st) {
    tg_bwd_live = false;
    if (!(train_graph && shape_ok && fwd_graphed && loss_staged && fwd_training && !prof.on)) return MIMO_OK;
    const uint64_t key = (tg_fwd_replay.live << 3) | (lmask ? 4 : 0) | (lperm ? 2 : 0) | (whole ? 1 : 0);
    const auto route = tg_bwd_replay.decide(key);
    if (route == sched::GraphReplayPolicy::Eager) return MIMO_OK;
    if (route == sched::GraphReplayPolicy::Capture) {
      for (auto& e : tg_bwd) destroy_exec(&e);
      // (a capture executes nothing: the stages can be captured one after the other, each on the host state — gradient
      // routing of the activation tensors — the stage before it left)
      const BwdCall staged{nullptr, g_dloss};
      int rc = MIMO_OK;
      if (whole) {
        rc = capture([&](hipStream_t cs) {
          ring.policy.rewind();
          for (int stage = 0; stage < kBwdStages; ++stage) MIMO_TRY(backward_stage(stage, staged, cs));
          return ring.join(cs);
        }, &tg_bwd[kBwdStages]);
      } else {
        for (int stage = 0; stage < kBwdStages && rc == MIMO_OK; ++stage)
          rc = capture([&](hipStream_t cs) {
            ring.policy.rewind();
            MIMO_TRY(backward_stage(stage, staged, cs));
            return ring.join(cs);
          }, &tg_bwd[stage]);
      }
      if (rc != MIMO_OK) {
        tg_bwd_replay.capture_failed();
        return rc;
      }
    }
    tg_bwd_live = true;
    MIMO_HIP_CHECK(hipMemcpyAsync(g_dloss, dloss, (size_t)S * sizeof(float), hipMemcpyDeviceToDevice, st));
    return MIMO_OK;
  }

  // the backward in progress replays graphs: the one of this stage range (every backward graph ends with the join of the side stream)
  int backward_replay(int stage_first, int stage_last, bool whole, bool graph_shaped, hipStream_t st) {
    if (!graph_shaped) {
      set_error("mimo_backward: stage %d..%d differs from what stage 0 of this backward was called with", stage_first, stage_last);
      return MIMO_ERR_STATE;
    }
    hipGraphExec_t e = whole ? tg_bwd[kBwdStages] : tg_bwd[stage_first];
    if (!e) {
      set_error("mimo_backward: no graph for stage range %d..%d of the backward in progress", stage_first, stage_last);
      return MIMO_ERR_STATE;
    }
    MIMO_HIP_CHECK(hipGraphLaunch(e, st));
    bwd_next_stage = stage_last + 1 < kBwdStages ? stage_last + 1 : 0;
    return MIMO_OK;
  }

  // the eager walk of the stages, then the hand-off: `ready` / ev_stage (see above), or the join
  int backward_eager(const BwdCall& call, int stage_first, int stage_last, hipStream_t* ready, hipStream_t st) {
    for (int stage = stage_first; stage <= stage_last; ++stage) MIMO_TRY(backward_stage(stage, call, st));
    bwd_next_stage = stage_last + 1 < kBwdStages ? stage_last + 1 : 0;
    if (ready && wg_async && !prof.on && stage_last < kBwdStages - 1) {
      MIMO_HIP_CHECK(hipEventRecord(ev_stage, st));
      MIMO_HIP_CHECK(hipStreamWaitEvent(ring.side, ev_stage, 0));
      *ready = ring.side;
      return MIMO_OK;
    }
    return ring.join(st);  // the gradients of the stages run so far are final for the caller (all-reduce)
  }

  int backward_stage(int stage, const BwdCall& call, hipStream_t st) {
    switch (stage) {
      case 0: {
        for (auto& dc : dcs) {
          dc->out.grad_writes = 0;
          dc->out.skipgrad = nullptr;
          dc->out.poolgrad = nullptr;
        }
        x2cat.grad_writes = 0;
        x2cat.skipgrad = nullptr;
        x2cat.poolgrad = nullptr;
        if (!fwd_training && !call.ig) {  // eval-mode forward skipped the dgrad weight packing
          MIMO_TRY(pack_all(true, st));
        }
        const int fp = pad_channels(f);
        for (int s = S - 1; s >= 0; --s) {
          DoubleConv* dc = up4[s];
          int rows = 0;
          const float* em = elem_masks[1 + s];
          if (fuse_bwd_head && Co == 2 && !dc->mask && !em && !elem_rng_on[1 + s]) {
            // the head's input gradient is formed by the BatchNorm backward of the decoder's last convolution itself (GS_HEAD):
            // head_bwd is not launched, the gradient of the decoder output is never written
            GradSrc hs;
            hs.kind = GS_HEAD;
            hs.head = HeadGrad{params + heads[s].off_w, f, Co, N, S, s, H * W, out, call.dout, call.dloss, label, lmask, lperm, cfg.loss_kind,
                               cfg.eps_min, cfg.eps_max, 1.f / (float)((double)N * (Co / 2) * H * W), s_headpart};
            MIMO_TRY(dc_backward(dc, true, call, st, &hs));
            if (call.ig) continue;  // (no head weight / bias gradient)
            // (the head's partial rows: one per workgroup of that reduction)
            MIMO_TRY(head_bwd_stats_launch(s_headpart, head_rows, f, fp, Co, grads + heads[s].off_w, grads + heads[s].off_b, st));
            continue;
          }
          const int blk = prof.begin(Profiler::kTierBase + 1, st);
          const int pr = prof.begin(MIMO_PROF_HEAD_BWD, st);
          // (the tensor the forward's head read: z through scale / shift + ReLU, or the materialised — possibly masked — one)
          const Act& o = dc->out;
          const bool oz = o.z_live;
          MIMO_TRY(head_bwd_launch(oz ? o.z : o.a, this->st, oz ? o.z_ld : o.ld, params + heads[s].off_w, f, fp, Co, N, S, s, H * W,
                                   out, call.dout, call.dloss, label, lmask, lperm, cfg.loss_kind, cfg.eps_min, cfg.eps_max, dc->out.da,
                                   s_partial, &rows, st, oz ? o.z_scale : nullptr, oz ? o.z_shift : nullptr));
          prof.end(pr, 0.0, 4.0 * (double)N * H * W * (2.0 * fp + Co + Co / 2), st);
          if (!call.ig)
            MIMO_TRY(head_bwd_stats_launch(s_partial, rows, f, fp, Co, grads + heads[s].off_w, grads + heads[s].off_b, st));
          if (em || elem_rng_on[1 + s]) {
            const ElemRng g = elem_rng(1 + s);
            MIMO_TRY(elem_mask_mul_launch(dc->out.da, this->st, dc->out.ldda, em, N, dc->out.C, dc->out.Cp, H * W, st,
                                          em ? nullptr : &g));
          }
          prof.end(blk, 0.0, 0.0, st);
          MIMO_TRY(dc_backward(dc, true, call, st));
        }
        return MIMO_OK;
      }
      case 1: return dc_backward(up3, true, call, st);
      case 2: return dc_backward(up2, true, call, st);
      case 3: return dc_backward(up1, true, call, st);
      case 4:
        {
          const float* em = elem_masks[0];
          if (em || elem_rng_on[0]) {
            const ElemRng g = elem_rng(0);
            MIMO_TRY(elem_mask_mul_launch(down4->out.da, this->st, down4->out.ldda, em, N, down4->out.C, down4->out.Cp,
                                          down4->out.H * down4->out.W, st, em ? nullptr : &g));
          }
        }
        return dc_backward(down4, true, call, st);
      case 5: return dc_backward(down3, true, call, st);
      case 6: return dc_backward(down2, true, call, st);
      default: return backward_encoders(call, st);
    }
  }

  // The 8 stages of the backward with the data-gradient chain only, the S first-layer data gradients folded and summed into
  // dimage [N,Ci,H,W] in the fixed order s = S-1, S-2, ..., 0 (fp32 adds; accumulate: on top of the caller's values).
  // replicas > 0 (mimo_input_gradient_mc): the batch is `replicas` passes of N / replicas images, pass-major; dimage
  // [N / replicas,Ci,H,W] receives, per encoder, the sum over its passes in the order m = 0 ... replicas-1.
  int input_gradient(const float* dout, const float* dloss, float* dimage, int accumulate, int replicas, hipStream_t st) {
    if (replicas < 0 || (replicas > 0 && N % replicas != 0)) {
      set_error("mimo_input_gradient_mc: replicas %d does not divide the plan batch %d (need replicas >= 1)", replicas, N);
      return MIMO_ERR_INVALID;
    }
    if (cfg.inference_only == 1 || !s_zero) {
      set_error("mimo_input_gradient: inference-only plan (no buffers for a backward)");
      return MIMO_ERR_STATE;
    }
    if (cfg.precision != MIMO_PREC_FP32 && cfg.precision != MIMO_PREC_SPLIT16) {
      set_error("mimo_input_gradient: implemented for the fp32 and split16 precisions, not for precision %d", cfg.precision);
      return MIMO_ERR_INVALID;
    }
    if (!dimage || (!dout && !dloss)) {
      set_error("mimo_input_gradient: need dimage and dout and/or dloss");
      return MIMO_ERR_INVALID;
    }
    if (!fwd_done || fwd_no_grad || fwd_training) {
      set_error("mimo_input_gradient: needs a mimo_forward with training = 0 and no_grad = 0 first");
      return MIMO_ERR_STATE;
    }
    if (had_perm) {
      set_error("mimo_input_gradient: needs a forward without perm");
      return MIMO_ERR_STATE;
    }
    if (dloss && !loss_done) {
      set_error("mimo_input_gradient: dloss given but mimo_loss_forward was not called");
      return MIMO_ERR_STATE;
    }
    if (bwd_next_stage != 0) {
      set_error("mimo_input_gradient: a staged mimo_backward is in progress (stage %d is next)", bwd_next_stage);
      return MIMO_ERR_STATE;
    }
    // the data-gradient weight images: packed once per parameter version (an eval-mode forward packs the forward images only)
    if (derived_version < 0 || dgrad_version != derived_version) {
      MIMO_TRY(pack_jobs_launch(pack_jobs + n_fwd_jobs, n_all_jobs - n_fwd_jobs, pack_max_total, params, st));
      dgrad_version = derived_version;
    }
    const BwdCall call{dout, dloss, nullptr, true, dimage, accumulate != 0, replicas};
    for (int stage = 0; stage < kBwdStages; ++stage) MIMO_TRY(backward_stage(stage, call, st));
    return MIMO_OK;
  }

  int backward_encoders(const BwdCall& call, hipStream_t st) {
    for (int s = S - 1; s >= 0; --s) MIMO_TRY(dc_backward(down1[s], true, call, st));
    for (int s = S - 1; s >= 0; --s) {
      MIMO_TRY(dc_backward(enc_in[s], call.dx != nullptr || call.ig, call, st));
      // s = S-1 assigns (or adds to the caller's values), S-2 ... 0 add: s_dxpadB is reused per encoder
      const int acc = (s < S - 1 || call.accumulate) ? 1 : 0;
      if (call.ig && call.replicas > 0)
        MIMO_TRY(fold_image_grad_mc_launch(s_dxpadB, Ci_p, N / call.replicas, call.replicas, Ci, H, W, call.dimage, acc, st));
      else if (call.ig)
        MIMO_TRY(fold_image_grad_launch(s_dxpadB, Ci_p, N, Ci, H, W, call.dimage, acc, st));
      else if (call.dx)
        MIMO_TRY(unpack_dx_launch(s_dxpadB, this->st, Ci_p, N, S, s, Ci, H, W, call.dx, st));
    }
    return MIMO_OK;
  }
};

// ======================================================================= C ABI ==========
extern "C" {

const char* mimo_last_error(void) { return mimo::last_error(); }
int mimo_version(void) { return 1; }

int mimo_plan_create(const mimo_config* cfg, mimo_plan** out) {
  if (!cfg || !out) {
    set_error("mimo_plan_create: null argument");
    return MIMO_ERR_INVALID;
  }
  MIMO_HIP_CHECK(hipSetDevice(cfg->device));
  auto p = std::make_unique<mimo_plan>();
  p->cfg = *cfg;
  const int rc = p->build();
  if (rc != MIMO_OK) return rc;
  MIMO_HIP_CHECK(hipDeviceSynchronize());
  *out = p.release();
  return MIMO_OK;
}

void mimo_plan_destroy(mimo_plan* plan) { delete plan; }
size_t mimo_plan_workspace_bytes(const mimo_plan* plan) { return plan ? plan->bytes : 0; }
int mimo_plan_num_tensors(const mimo_plan* plan) { return plan ? (int)plan->tensors.size() : 0; }
int64_t mimo_plan_param_floats(const mimo_plan* plan) { return plan ? plan->param_floats : 0; }
int64_t mimo_plan_buffer_floats(const mimo_plan* plan) { return plan ? plan->buffer_floats : 0; }
int mimo_plan_num_double_convs(const mimo_plan* plan) { return plan ? (int)plan->dcs.size() : 0; }
int mimo_plan_double_conv_channels(const mimo_plan* plan, int index) {
  if (!plan || index < 0 || index >= (int)plan->dcs.size()) return -1;
  return plan->dcs[index]->c2.Cout;
}

int mimo_plan_tensor_info(const mimo_plan* plan, int index, char* name, int name_cap, int64_t shape[4], int* ndim,
                          int* kind, int64_t* offset) {
  if (!plan || index < 0 || index >= (int)plan->tensors.size()) {
    set_error("mimo_plan_tensor_info: bad index");
    return MIMO_ERR_INVALID;
  }
  const TensorInfo& t = plan->tensors[index];
  if (name && name_cap > 0) {
    strncpy(name, t.name.c_str(), name_cap - 1);
    name[name_cap - 1] = 0;
  }
  if (shape)
    for (int i = 0; i < 4; ++i) shape[i] = t.shape[i];
  if (ndim) *ndim = t.ndim;
  if (kind) *kind = t.kind;
  if (offset) *offset = t.offset;
  return MIMO_OK;
}

int mimo_plan_bind(mimo_plan* plan, float* params, float* grads, float* bn_buffers) {
  if (!plan || !params || !bn_buffers) {
    set_error("mimo_plan_bind: null argument");
    return MIMO_ERR_INVALID;
  }
  if (plan->params != params || plan->bnbuf != bn_buffers) {
    plan->derived_version = -1;  // other tensors: re-derive
    plan->dgrad_version = -1;
    plan->drop_graphs();         // the captured kernels hold the old parameter pointers
  }
  if (plan->grads != grads) plan->drop_graphs();
  plan->params = params;
  plan->grads = grads;
  plan->bnbuf = bn_buffers;
  return MIMO_OK;
}

int mimo_plan_status(mimo_plan* plan, int32_t* flags, int32_t clear, mimo_stream stream) {
  if (!plan || !flags) {
    set_error("mimo_plan_status: bad argument");
    return MIMO_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  int v = 0;
  MIMO_HIP_CHECK(hipMemcpyAsync(&v, plan->d_status, sizeof(int), hipMemcpyDeviceToHost, st));
  if (clear) MIMO_HIP_CHECK(hipMemsetAsync(plan->d_status, 0, sizeof(int), st));
  MIMO_HIP_CHECK(hipStreamSynchronize(st));
  *flags = v;
  return MIMO_OK;
}

int mimo_plan_dropout_mask(mimo_plan* plan, int site, float* dst, mimo_stream stream) {
  if (!plan || !dst || site < 0 || site >= (int)plan->dcs.size() + 1 + plan->S) {
    set_error("mimo_plan_dropout_mask: bad argument");
    return MIMO_ERR_INVALID;
  }
  const int ndc = (int)plan->dcs.size();
  if (site < ndc) {  // Dropout2d: the multipliers the last forward used (drawn in the engine or staged from the caller)
    const float* src = plan->dcs[site]->mask;
    const size_t n = (size_t)plan->N * plan->dcs[site]->c2.Cout;
    if (!src) {
      set_error("mimo_plan_dropout_mask: site %d had no mask in the last forward", site);
      return MIMO_ERR_STATE;
    }
    MIMO_HIP_CHECK(hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return MIMO_OK;
  }
  const int j = site - ndc;
  if (!plan->elem_rng_on[j]) {
    set_error("mimo_plan_dropout_mask: element-wise site %d was not drawn by the engine in the last forward", j);
    return MIMO_ERR_STATE;
  }
  const Act& o = j == 0 ? plan->down4->out : plan->up4[j - 1]->out;
  const ElemRng g = plan->elem_rng(j);
  return elem_dropout_mask_launch(dst, plan->N, o.C, o.Cp, o.H * o.W, g.site, g.seed, g.offset, g.p, (hipStream_t)stream);
}

int mimo_plan_profile(mimo_plan* plan, int enable) {
  if (!plan) {
    set_error("mimo_plan_profile: null plan");
    return MIMO_ERR_INVALID;
  }
  MIMO_TRY(plan->prof.collect());
  plan->prof.on = enable != 0;
  if (enable) plan->prof.clear_totals();
  return MIMO_OK;
}

int mimo_plan_profile_read(mimo_plan* plan, int kind, double* total_ms, int64_t* launches, double* flops, double* bytes) {
  if (!plan || kind < 0 || kind >= MIMO_PROF_KINDS) {
    set_error("mimo_plan_profile_read: bad argument");
    return MIMO_ERR_INVALID;
  }
  MIMO_TRY(plan->prof.collect());
  if (total_ms) *total_ms = plan->prof.ms[kind];
  if (launches) *launches = plan->prof.launches[kind];
  if (flops) *flops = plan->prof.flops[kind];
  if (bytes) *bytes = plan->prof.bytes[kind];
  return MIMO_OK;
}

int mimo_plan_profile_read_tier(mimo_plan* plan, int tier, double* forward_ms, double* backward_ms) {
  if (!plan || tier < 0 || tier >= Profiler::kTiers) {
    set_error("mimo_plan_profile_read_tier: bad argument");
    return MIMO_ERR_INVALID;
  }
  MIMO_TRY(plan->prof.collect());
  if (forward_ms) *forward_ms = plan->prof.tier_ms[2 * tier];
  if (backward_ms) *backward_ms = plan->prof.tier_ms[2 * tier + 1];
  return MIMO_OK;
}

int mimo_plan_profile_read_kind_tier(mimo_plan* plan, int kind, int tier, double* ms) {
  if (!plan || kind < 0 || kind >= MIMO_PROF_KINDS || tier < 0 || tier >= Profiler::kTiers || !ms) {
    set_error("mimo_plan_profile_read_kind_tier: bad argument");
    return MIMO_ERR_INVALID;
  }
  MIMO_TRY(plan->prof.collect());
  *ms = plan->prof.kind_tier_ms[kind][tier];
  return MIMO_OK;
}

int mimo_forward(mimo_plan* plan, const mimo_forward_args* args, mimo_stream stream) {
  if (!plan) {
    set_error("mimo_forward: null plan");
    return MIMO_ERR_INVALID;
  }
  return plan->forward(args, (hipStream_t)stream);
}

int mimo_loss_forward(mimo_plan* plan, const float* label, const float* mask, const int64_t* perm, float* loss_out,
                      mimo_stream stream) {
  if (!plan) {
    set_error("mimo_loss_forward: null plan");
    return MIMO_ERR_INVALID;
  }
  return plan->loss_forward(label, mask, perm, loss_out, (hipStream_t)stream);
}

int mimo_backward(mimo_plan* plan, const float* dout, const float* dloss, float* dx, mimo_stream stream) {
  if (!plan) {
    set_error("mimo_backward: null plan");
    return MIMO_ERR_INVALID;
  }
  return plan->backward(dout, dloss, dx, 0, mimo_plan::kBwdStages - 1, (hipStream_t)stream);
}

int mimo_backward_stage(mimo_plan* plan, int stage, const float* dout, const float* dloss, float* dx, mimo_stream stream) {
  if (!plan) {
    set_error("mimo_backward_stage: null plan");
    return MIMO_ERR_INVALID;
  }
  return plan->backward(dout, dloss, dx, stage, stage, (hipStream_t)stream);
}

int mimo_backward_stage_async(mimo_plan* plan, int stage, const float* dout, const float* dloss, float* dx, mimo_stream stream,
                              mimo_stream* ready_stream) {
  if (!plan || !ready_stream) {
    set_error("mimo_backward_stage_async: null argument");
    return MIMO_ERR_INVALID;
  }
  hipStream_t ready = nullptr;
  const int rc = plan->backward(dout, dloss, dx, stage, stage, (hipStream_t)stream, &ready);
  *ready_stream = (mimo_stream)ready;
  return rc;
}

int mimo_input_gradient(mimo_plan* plan, const float* dout, const float* dloss, float* dimage, int accumulate, mimo_stream stream) {
  if (!plan) {
    set_error("mimo_input_gradient: null plan");
    return MIMO_ERR_INVALID;
  }
  return plan->input_gradient(dout, dloss, dimage, accumulate, 0, (hipStream_t)stream);
}

int mimo_input_gradient_mc(mimo_plan* plan, const float* dout, const float* dloss, float* dimage, int accumulate, int replicas,
                           mimo_stream stream) {
  if (!plan) {
    set_error("mimo_input_gradient_mc: null plan");
    return MIMO_ERR_INVALID;
  }
  if (replicas < 1) {
    set_error("mimo_input_gradient_mc: replicas %d (need replicas >= 1)", replicas);
    return MIMO_ERR_INVALID;
  }
  return plan->input_gradient(dout, dloss, dimage, accumulate, replicas, (hipStream_t)stream);
}

int64_t mimo_plan_encoder_param_floats(const mimo_plan* plan) { return plan ? plan->encoder_param_floats : 0; }

int mimo_plan_num_backward_stages(const mimo_plan* plan) { return plan ? mimo_plan::kBwdStages : 0; }

int mimo_plan_backward_stage_range(const mimo_plan* plan, int stage, int64_t* begin, int64_t* end) {
  if (!plan || stage < 0 || stage >= mimo_plan::kBwdStages || !begin || !end) {
    set_error("mimo_plan_backward_stage_range: bad argument");
    return MIMO_ERR_INVALID;
  }
  plan->stage_range(stage, begin, end);
  return MIMO_OK;
}

}  // extern "C"
