// The SPLIT-VAE (LGVae) training step as one native launch sequence.
//
// Replaces LGVae.call (vae/model.py:189-200) + train_step_lg_vae (vae/trainer.py:120-144) +
// Adam.apply_gradients (vae/main.py:65): weight preparation, both encoders, reparameterisation/KL,
// both decoders, discretised-logistic ELBO, the full backward pass and the Keras-Adam update are
// enqueued on one HIP stream from C++ (no Python per kernel), over a caller-owned workspace.
// The phase mask lets the data-parallel driver slip its RCCL all-reduce between the decoder
// backward, the encoder backward and Adam.
#include <string>
#include <algorithm>
#include <vector>
#include <map>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "common.hip.h"
#include "kernels.h"
#include "conv_geom.h"
#include "buffer_table.h"
#include "plan_streams.h"
#include "plan_profile.h"
#include "plan_latent.h"

namespace {

// THE workspace buffer list: id, public name (sv_lgvae_buffer) and position in the workspace, in this order.  ONE: a single buffer.  TWIN: one kind per
// network -- id = the x network's buffer `<name>x`, id + 1 = the x-hat network's `<name>xh` right behind it (exactly `bytes` behind when the size is a multiple of
// 256 B, so pointwise kernels can take both as one batch of 2B: the run-time `contig` test of phase_bwd_decoders).
// A buffer that a plan's mode lacks has NO offset and a NULL pointer (build_buffers):
//   - global_only (GMVae) has no x-hat network and no encoder of its own: none of the x-hat buffers but in8_xh, none of a1_ .. ga1_ but gz_x.  Its phases never
//     touch them, with ONE exception that reads the nulls on purpose: phase_loss hands nll / kl / nllpart of the x-hat network and kl_x to svk_finalize_losses,
//     which reads a null term as zero;
//   - polycw2_ .. polycw4_ (dW' + frame slabs of the fp32 polyphase weight gradient of dec[][2 .. 4]) exist only where svk_polyc_wgrad_ws_floats() asks for
//     them: run_wgrad_layers takes that form only where has() says so.
// pre_ .. gz_ are zeroed every step by ONE memset (split-K / atomic accumulation targets), gz_ alone by another: BufTable::run() at creation.
#define LGVAE_BUFFERS(ONE, TWIN) \
  ONE(JOBS, "jobs") ONE(WARENA, "warena") ONE(WGRAD_WS, "wgrad_ws") TWIN(POLYFIX, "polyfix_") TWIN(POLYCFIX, "polycfix_") TWIN(POLYD, "polyd_") \
  TWIN(POLYCW2, "polycw2_") TWIN(POLYCW3, "polycw3_") TWIN(POLYCW4, "polycw4_") TWIN(POLYW, "polyw_") TWIN(LAT_WS, "lat_ws_") \
  ONE(DYN, "dyn") ONE(LOSSES, "losses") ONE(METRIC_ACC, "metric_acc") ONE(ZCAT, "zcat") TWIN(IN8, "in8_") \
  TWIN(A1, "a1_") TWIN(A2, "a2_") TWIN(A3, "a3_") TWIN(PRE, "pre_") TWIN(GZ, "gz_") TWIN(Z_MEAN, "z_mean_") TWIN(Z_SIG, "z_sig_") TWIN(Z, "z_") \
  TWIN(EPS, "eps_") TWIN(KL, "kl_") TWIN(GHEAD, "ghead_") TWIN(GA3, "ga3_") TWIN(GA2, "ga2_") TWIN(GA1, "ga1_") \
  TWIN(H1, "h1_") TWIN(H2, "h2_") TWIN(U2, "u2_") TWIN(H3, "h3_") TWIN(U3, "u3_") TWIN(H4, "h4_") TWIN(U4, "u4_") TWIN(OUT6, "out6_") TWIN(NLL, "nll_") \
  TWIN(NLLPART, "nllpart_") TWIN(G5, "g5_") TWIN(GU4, "gu4_") TWIN(G4, "g4_") TWIN(GU3, "gu3_") TWIN(G3, "g3_") TWIN(GU2, "gu2_") TWIN(G2, "g2_") TWIN(G1, "g1_")
enum BufId {
#define ONE(id, name) id,
#define TWIN(id, name) id, id##_XH,
  LGVAE_BUFFERS(ONE, TWIN)
#undef ONE
#undef TWIN
  NBUF
};
static_assert(POLYCW4_XH < 32, "Layer::polycw is also a bit of sv_lgvae_plan::polycw_bad");
typedef void* const* BufPair;     // {x, x-hat} of a TWIN kind
const char* const BUF_NAMES[NBUF] = {
#define ONE(id, name) name,
#define TWIN(id, name) name "x", name "xh",
  LGVAE_BUFFERS(ONE, TWIN)
#undef ONE
#undef TWIN
};

struct ParamInfo { std::string name; int64_t off; int ndim; int64_t shape[4]; int64_t count; };

static std::vector<ParamInfo> build_params(const sv_lgvae_desc* d) {
  std::vector<ParamInfo> v;
  int64_t off = 0;
  auto add = [&](const std::string& n, std::initializer_list<int64_t> shp) {
    ParamInfo p;
    p.name = n; p.off = off; p.ndim = (int)shp.size(); p.count = 1;
    int i = 0;
    for (auto s : shp) { p.shape[i++] = s; p.count *= s; }
    for (; i < 4; ++i) p.shape[i] = 1;
    off += (p.count + 3) / 4 * 4;   // keep every tensor 16-B aligned in the flat buffer
    v.push_back(p);
  };
  const int64_t F = (int64_t)(d->H / 8) * (d->W / 8) * 128;
  // vae/model.py:152 writes image_shape[1]//8*image_shape[2]//8*128 = ((H//8)*W)//8*128
  const int64_t D1 = ((int64_t)(d->H / 8) * d->W) / 8 * 128;
  auto enc = [&](const std::string& pre, int64_t L) {
    add(pre + "/e1/kernel", {6, 6, 3, 32}); add(pre + "/e1/bias", {32});
    add(pre + "/e2/kernel", {6, 6, 32, 64}); add(pre + "/e2/bias", {64});
    add(pre + "/e3/kernel", {4, 4, 64, 128}); add(pre + "/e3/bias", {128});
    add(pre + "/e4_mean/kernel", {F, L}); add(pre + "/e4_mean/bias", {L});
    add(pre + "/e4_sd/kernel", {F, L}); add(pre + "/e4_sd/bias", {L});
  };
  auto dec = [&](const std::string& pre, int64_t L) {
    add(pre + "/d1/kernel", {L, D1}); add(pre + "/d1/bias", {D1});
    add(pre + "/d2/kernel", {4, 4, 128, 128}); add(pre + "/d2/bias", {128});
    add(pre + "/d3/kernel", {4, 4, 128, 64}); add(pre + "/d3/bias", {64});
    add(pre + "/d4/kernel", {6, 6, 64, 32}); add(pre + "/d4/bias", {32});
    add(pre + "/d5/kernel", {6, 6, 32, 6}); add(pre + "/d5/bias", {6});
  };
  if (d->global_only) {                 // GMVae: decoder_x over z_x alone (vae/model.py:285-286)
    dec("decoder_x", d->global_latent);
    return v;
  }
  enc("encoder_x", d->global_latent);
  enc("encoder_x_hat", d->local_latent);
  dec("decoder_x", d->global_latent + d->local_latent);
  dec("decoder_x_hat", d->local_latent);
  return v;
}

static int check_desc(const sv_lgvae_desc* d) {
  if (!d) return SV_E_BADARG;
  if (d->B <= 0 || d->H < 8 || d->W < 8) return SV_E_BADARG;
  if (d->H != d->W || ilog2_exact(d->H) < 0) return SV_E_UNSUPPORTED;
  if (d->global_only && !d->external_global_encoder) return SV_E_BADARG;   // the one branch's encoder is the caller's
  if (d->global_only) {                                                    // (local_latent is ignored)
    if (d->global_latent <= 0) return SV_E_BADARG;
    if (ilog2_exact(d->global_latent) < 0 || d->global_latent < 8) return SV_E_UNSUPPORTED;
    if (d->dtype != SV_BF16 && d->dtype != SV_F32) return SV_E_BADARG;
    return SV_OK;
  }
  if (d->global_latent <= 0 || d->local_latent <= 0) return SV_E_BADARG;
  if (ilog2_exact(d->global_latent) < 0 || ilog2_exact(d->local_latent) < 0 || d->global_latent < 8 ||
      d->local_latent < 8 || d->global_latent != d->local_latent)
    return SV_E_UNSUPPORTED;   // MFMA K-pieces want power-of-two channel counts (reference default 128/128)
  if (d->dtype != SV_BF16 && d->dtype != SV_F32) return SV_E_BADARG;
  return SV_OK;
}

// one conv-like layer instance with everything needed for fwd / dgrad / wgrad
struct Layer {
  std::string ln, sc_fwd, sc_dgrad, sc_wgrad, sc_reduce;   // "d4" and its profile scopes "fwd.d4", "dgrad.d4", "wgrad.d4", "wgrad.d4.reduce" (build_layers)
  int polycw = -1;              // dec[][2 .. 4]: the TWIN id of its polyphase weight-gradient workspace (POLYCW2 ..), which the plan may lack; and its bit in polycw_bad
  sv_conv_desc d;
  int kparam, bparam;           // indices into the param table (kernel, bias); head uses two kernels
  // element offsets in the arena, filled from the layout table (conv_geom.h: WImage) when the images are placed (build_prep_jobs)
  int64_t wf_off;               // forward image
  int64_t wfix_off;             // border-fix image of the polyphase head (svg_poly), or -1
  int64_t wd_off[4];            // input-gradient image: per parity class (wd_off[0] = the image's base)
  bool polyd;                   // the input-gradient image has the polyphase parts (svg_polyd: main / edge / corner), LATCHED like polyc
  bool need_dgrad;
  bool polyc;                   // forward in per-class polyphase form (conv_geom.h: svg_polyc), LATCHED when the plan is created: the arena then holds the class images
                                // only, and a later change of the tuning environment must not send the direct kernel to them
};

}  // namespace

struct sv_lgvae_plan {
  sv_lgvae_desc d;
  std::vector<ParamInfo> params;
  int64_t nparams;
  BufTable<NBUF> bufs{BUF_NAMES};
  bool bound;
  // layers: [enc_x e1,e2,e3,head][enc_xh ...][dec_x d1..d5][dec_xh ...]
  Layer enc[2][4];
  Layer dec[2][5];
  std::vector<PrepJob> jobs;
  int prep_blocks;
  int dec_block0 = 0;           // first block of the decoders' jobs in the table (the encoders' jobs come first): the step prepares the two halves on two streams
  int64_t arena_elems;
  bool nll_fused = false;  // the last decoder forward evaluated the loss in the head's epilogue (nllpart_*, g5_* are valid)
  LatentBlock lat;              // where dL/dz lives (DzState), the latched launch forms and the K-slice geometry: plan_latent.h
  unsigned polycw_bad = 0;      // decoder layers (bit = Layer::polycw) whose polyphase weight gradient was refused once: not tried again (one profile scope per launch)
  SideStreams side;             // weight-gradient / early side streams, their fork / join / bucket events and test hooks: plan_streams.h
  Profiler prof;                // per-scope hipEvent timing: plan_profile.h
  // captured steps (sv_lgvae_graph_enable): one executable graph per distinct (phase mask, buffers, baked scalars)
  bool graph_on = false;
  const SvDynArgs* dyn = nullptr;   // non-null while a step is being captured
  // host-side state that a phase reads on entry and leaves behind on exit: it selects launches (which buffer reparam_kl_bwd reads, whether dz is
  // re-zeroed, whether the ELBO gradient comes from the fused head), so it is part of a captured graph's key and a replay must leave the
  // plan in the state the captured phases left it in
  struct HostState { DzState dz; bool nll_fused; };
  HostState host_state() const { return {lat.dz, nll_fused}; }
  void set_host_state(const HostState& h) { lat.dz = h.dz; nll_fused = h.nll_fused; }
  uint64_t host_state_bits() const { return (uint64_t)lat.dz | (uint64_t)nll_fused << 2; }
  struct GraphEntry { hipGraphExec_t exec = nullptr; int seen = 0; HostState exit_state{}; };
  std::map<std::vector<uint64_t>, GraphEntry> graphs;

  size_t esz() const { return d.dtype == SV_BF16 ? 2 : 4; }
  int ndec() const { return d.global_only ? 1 : 2; }                       // decoders (and x / x-hat networks) the plan runs
  int lc() const { return d.global_only ? d.global_latent : d.global_latent + d.local_latent; }   // decoder_x's input width = zcat / gz_x pitch
  // k picks the network of a TWIN buffer: 0 = x, 1 = x-hat
  void* buf(int id, int k = 0) const { return bufs.ptr[id + k]; }
  BufPair pair(int id) const { return &bufs.ptr[id]; }                   // as the twin launches take them
  float* const* fpair(int id) const { return (float* const*)pair(id); }
  int64_t bbytes(int id, int k = 0) const { return bufs.bytes[id + k]; }
};

namespace {

// A/B: one launch per network for the small pointwise kernels (Sampling + KL and their adjoints) instead of one for the x / x-hat twins
static bool no_twin_pointwise() { static const bool v = SV_TUNE_FLAG("SV_NO_TWIN_POINTWISE"); return v; }

static void build_layers(sv_lgvae_plan* p) {
  const sv_lgvae_desc& d = p->d;
  const int H = d.H, W = d.W, B = d.B;
  const int F = (H / 8) * (W / 8) * 128;
  const int Lg = d.global_latent, Ll = d.local_latent;
  auto mk = [&](const std::string& name, int h, int w, int cin, int cout, int k, int s, int act, int ldx,
                int ldy, int yf32, int kparam, bool need_dgrad) {
    Layer L;
    L.ln = name; L.sc_fwd = "fwd." + name; L.sc_dgrad = "dgrad." + name; L.sc_wgrad = "wgrad." + name; L.sc_reduce = L.sc_wgrad + ".reduce";
    L.d = sv_conv_desc{B, h, w, cin, cout, k, k, s, act, d.dtype, ldx, ldy, yf32, 0};
    L.kparam = kparam; L.bparam = kparam + 1; L.need_dgrad = need_dgrad;
    L.wf_off = 0; L.wfix_off = -1; L.polyd = false; L.polyc = false;
    for (int i = 0; i < 4; ++i) L.wd_off[i] = 0;
    return L;
  };
  for (int e = 0; e < 2 && !d.global_only; ++e) {
    const int pb = e * 10;
    const int L = e == 0 ? Lg : Ll;
    p->enc[e][0] = mk("e1", H, W, 3, 32, 6, 2, SV_ACT_RELU, 8, 32, 0, pb + 0, false);
    p->enc[e][1] = mk("e2", H / 2, W / 2, 32, 64, 6, 2, SV_ACT_RELU, 32, 64, 0, pb + 2, true);
    p->enc[e][2] = mk("e3", H / 4, W / 4, 64, 128, 4, 2, SV_ACT_RELU, 64, 128, 0, pb + 4, true);
    // e4_mean | e4_sd as ONE dense GEMM with N = 2L (vae/model.py:41-42,:111-112)
    p->enc[e][3] = mk("head", 1, 1, F, 2 * L, 1, 1, SV_ACT_NONE, F, 2 * L, 1, pb + 6, true);
  }
  for (int k = 0; k < p->ndec(); ++k) {
    const int pb = d.global_only ? 0 : 20 + k * 10;
    const int Lz = k == 0 ? p->lc() : Ll;
    p->dec[k][0] = mk("d1", 1, 1, Lz, F, 1, 1, SV_ACT_RELU, p->lc(), F, 0, pb + 0, true);
    p->dec[k][1] = mk("d2", H / 8, W / 8, 128, 128, 4, 1, SV_ACT_RELU, 128, 128, 0, pb + 2, true);
    p->dec[k][2] = mk("d3", H / 4, W / 4, 128, 64, 4, 1, SV_ACT_RELU, 128, 64, 0, pb + 4, true);
    p->dec[k][3] = mk("d4", H / 2, W / 2, 64, 32, 6, 1, SV_ACT_RELU, 64, 32, 0, pb + 6, true);
    p->dec[k][4] = mk("d5", H, W, 32, 6, 6, 1, SV_ACT_NONE, 32, 6, 1, pb + 8, true);
    // the three bilinear resizes are fused into the staging of d3/d4/d5's forward and wgrad tiles (needs >= 16 output pixels per image for
    // the tile kernels: any H >= 16 here); fp32 since round 4 too (wgrad_tile_f32.hip; SV_F32_MATERIALISE_UPSAMPLE=1: u2 / u3 / u4 written out)
    static const bool no_fuse = SV_TUNE_FLAG("SV_NO_FUSED_UPSAMPLE");
    static const bool f32_mat = SV_TUNE_FLAG("SV_F32_MATERIALISE_UPSAMPLE");
    if ((d.dtype == SV_BF16 || !f32_mat) && !no_fuse && H >= 16)
      for (int l = 2; l <= 4; ++l) p->dec[k][l].d.ups_in = 1;
    for (int l = 2; l <= 4; ++l) p->dec[k][l].polycw = POLYCW2 + 2 * (l - 2);
  }
}

static void build_prep_jobs(sv_lgvae_plan* p) {
  PrepArena ar;
  auto do_layer = [&](Layer& L, bool is_head) {
    if (!is_head) {
      // per-class polyphase forward (conv_geom.h: svg_polyc) where the class problems plan on the tile kernel, else the direct form; the input / weight
      // gradients keep their own forms whichever forward image was prepared
      L.polyc = svg_polyc(&L.d) && svk_polyc_fwd_plannable(&L.d);
      const int64_t src = p->params[L.kparam].off;
      WImage w;
      svg_wimage_fwd(&L.d, L.polyc, false, &w);
      L.wf_off = ar.place(w, src);
      if (const WImagePart* fix = w.find(SV_WP_POLY_FIX)) L.wfix_off = L.wf_off + fix->off;
      if (!L.need_dgrad) return;
      svg_wimage_dgrad(&L.d, &w);
      const int64_t base = ar.place(w, src);
      for (int c = 0; c < svg_dgrad_classes(&L.d); ++c) L.wd_off[c] = base + w.off(SV_WP_DGRAD_CLASS, c);
      L.polyd = w.find(SV_WP_POLYD_MAIN) != nullptr;
    } else {
      // two Keras tensors [F,L] (mean at kparam, sd at kparam+2) -> one [2L][F] forward image
      // and one [F][2L] dgrad image
      const int F = L.d.Cin, L2 = L.d.Cout, Lh = L2 / 2;
      ar.align(); L.wf_off = ar.elems;
      for (int h = 0; h < 2; ++h) {
        PrepJob j;
        memset(&j, 0, sizeof(j));
        j.src_off = p->params[L.kparam + 2 * h].off;
        j.ntaps = 1; j.Cin = F; j.Cout = Lh; j.rows = Lh; j.inner = F; j.inner_ld = F; j.inner_off = 0;
        j.transpose = 0; j.srctap[0] = 0;
        j.dst_off = ar.elems + (int64_t)h * Lh * F;
        j.nblocks = svg_prep_nblocks(&j);
        ar.push(j);
      }
      ar.elems += (int64_t)L2 * F;
      ar.align(); L.wd_off[0] = ar.elems;
      for (int h = 0; h < 2; ++h) {
        PrepJob j;
        memset(&j, 0, sizeof(j));
        j.src_off = p->params[L.kparam + 2 * h].off;
        j.ntaps = 1; j.Cin = F; j.Cout = Lh; j.rows = F; j.inner = Lh; j.inner_ld = L2; j.inner_off = h * Lh;
        j.transpose = 1; j.srctap[0] = 0;
        j.dst_off = ar.elems;
        j.nblocks = svg_prep_nblocks(&j);
        ar.push(j);
      }
      ar.elems += (int64_t)F * L2;
    }
  };
  for (int e = 0; e < 2 && !p->d.global_only; ++e)
    for (int l = 0; l < 4; ++l) do_layer(p->enc[e][l], l == 3);
  p->dec_block0 = ar.blocks;
  for (int k = 0; k < p->ndec(); ++k)
    for (int l = 0; l < 5; ++l) do_layer(p->dec[k][l], false);
  p->arena_elems = ar.elems + 128;
  p->prep_blocks = ar.blocks;
  p->jobs = std::move(ar.jobs);
}

// sizes by id; LGVAE_BUFFERS gives the positions (the order of the statements here gives nothing)
static void build_buffers(sv_lgvae_plan* p) {
  const sv_lgvae_desc& d = p->d;
  const int64_t B = d.B, H = d.H, W = d.W, es = (int64_t)p->esz();
  const int64_t F = (H / 8) * (W / 8) * 128;
  const int Lg = d.global_latent, Ll = d.local_latent, Lc = p->lc();
  const bool go = d.global_only;           // GMVae: no x-hat network, no encoder of the plan's own -- none of their buffers
  int64_t sz[NBUF];
  for (auto& v : sz) v = -1;
  auto twin = [&](int id, int64_t bytes_x, int64_t bytes_xh) {
    sz[id] = bytes_x;
    if (!go) sz[id + 1] = bytes_xh;
  };
  auto same = [&](int id, int64_t bytes) { twin(id, bytes, bytes); };
  sz[JOBS] = (int64_t)p->jobs.size() * sizeof(PrepJob);
  sz[WARENA] = p->arena_elems * es;
  sz[WGRAD_WS] = SV_WGRAD_WS_BYTES * SV_WGRAD_MAX_MULTI * SideStreams::SIDE_MAX;   // per side stream, per problem
  same(POLYFIX, svk_poly_fix_ws_bytes((int)B, (int)H / 2, (int)W / 2));   // border terms of the polyphase head (poly_fix.hip)
  {   // border terms of the per-class polyphase layers (d3, d4): one region per network, sized for the largest layer (the layers run one after the other)
    int64_t need = 256;
    for (int l = 2; l <= 4; ++l)
      if (p->dec[0][l].polyc) need = std::max<int64_t>(need, svg_polyc_fix_ws_bytes(&p->dec[0][l].d));
    same(POLYCFIX, need);
    int64_t needd = 256;                                  // edge terms of the polyphase input gradients (d4, d5): one region per network
    for (int l = 2; l <= 4; ++l)
      if (svg_polyd(&p->dec[0][l].d)) needd = std::max<int64_t>(needd, svg_polyd_ws_bytes(&p->dec[0][l].d));
    same(POLYD, needd);
    // polyphase weight gradients at fp32 (polyc_wgrad.hip): dW' + frame slabs per layer and network (the layers' launches may overlap across streams)
    for (int l = 2; l <= 4; ++l) {
      const int64_t fl = svk_polyc_wgrad_ws_floats(&p->dec[0][l].d);
      if (fl) same(p->dec[0][l].polycw, fl * 4);
    }
  }
  same(POLYW, svk_poly_wgrad_ws_floats(32, SV_POLY_WGRAD_NWG) * 4);        // polyphase weight gradient of the head: dW', dbias', frame slabs
  {   // K-slice slabs of the heads' forward and d1's input gradient (latent_gemm.hip): [S][B][N] fp32 per network
    const int64_t Fd = (H / 8) * (W / 8) * 128;
    // the four launches that write them -- heads of x / x-hat (N = 2 Lg / 2 Ll), d1's input gradient of decoder_x / decoder_x-hat (N = Lg + Ll / Ll) --
    // pick their split PER PROBLEM: sized as the maximum of the four actual (split, N) products (with unequal latent sizes a
    // per-problem split x N could exceed a product formed from two of them).  The splits and slab strides are FIXED here: the launch sites and
    // Sampling + KL read p->lat, so what is launched is what was sized
    LatentBlock& lat = p->lat;
    int64_t need = 0;
    auto slabs = [&](int64_t Nq, int* S, int64_t* stride) {
      *S = svk_nt_gemm_pick_splitk((int)B, (int)Nq, (int)Fd, 2);
      *stride = B * Nq;
      need = std::max<int64_t>(need, *S * *stride * 4);
    };
    for (int k = 0; k < p->ndec(); ++k) {
      if (!go) slabs(2 * (k == 0 ? Lg : Ll), &lat.head_S[k], &lat.head_stride[k]);     // (GMVae: d1's input gradient only, N = Lg)
      slabs(k == 0 ? Lc : Ll, &lat.d1_S[k], &lat.d1_stride[k]);
    }
    same(LAT_WS, need);
  }
  sz[DYN] = sizeof(SvDynArgs);
  sz[LOSSES] = sz[METRIC_ACC] = 8 * 4;
  sz[ZCAT] = B * Lc * es;
  sz[IN8] = sz[IN8_XH] = B * H * W * 8 * es;     // (global_only too: the split pass and the staged augmentation write both halves of images6)
  if (go) {
    sz[GZ] = B * Lc * 4;                         // dL/dz_x for the caller's encoder
  } else {
    same(A1, B * (H / 2) * (W / 2) * 32 * es);
    same(A2, B * (H / 4) * (W / 4) * 64 * es);
    same(A3, B * F * es);
    twin(PRE, B * 2 * Lg * 4, B * 2 * Ll * 4);
    twin(GZ, B * Lc * 4, B * Ll * 4);
    twin(Z_MEAN, B * Lg * 4, B * Ll * 4);
    twin(Z_SIG, B * Lg * 4, B * Ll * 4);
    twin(Z, B * Lg * 4, B * Ll * 4);
    twin(EPS, B * Lg * 4, B * Ll * 4);
    same(KL, B * 4);
    twin(GHEAD, B * 2 * Lg * es, B * 2 * Ll * es);
    same(GA3, B * F * es);
    same(GA2, B * (H / 4) * (W / 4) * 64 * es);
    same(GA1, B * (H / 2) * (W / 2) * 32 * es);
  }
  // decoders
  same(H1, B * F * es);
  same(H2, B * F * es);
  same(U2, B * (H / 4) * (W / 4) * 128 * es);
  same(H3, B * (H / 4) * (W / 4) * 64 * es);
  same(U3, B * (H / 2) * (W / 2) * 64 * es);
  same(H4, B * (H / 2) * (W / 2) * 32 * es);
  same(U4, B * H * W * 32 * es);
  same(OUT6, B * H * W * 6 * 4);
  same(NLL, B * 4);
  same(NLLPART, sv_dlogistic_nll_workspace_bytes((int)B, (int)H, (int)W));
  same(G5, B * H * W * 8 * es);
  same(GU4, B * H * W * 32 * es);
  same(G4, B * (H / 2) * (W / 2) * 32 * es);
  same(GU3, B * (H / 2) * (W / 2) * 64 * es);
  same(G3, B * (H / 4) * (W / 4) * 64 * es);
  same(GU2, B * (H / 4) * (W / 4) * 128 * es);
  same(G2, B * F * es);
  same(G1, B * F * es);
  p->bufs.layout(sz);
}

// the latent block's GEMMs on latent_gemm.hip (LDS-DMA phases, split-K through fp32 slabs summed in slice order) instead of the im2col
// kernel's split-K atomics; SV_NO_LATENT_GEMM restores the old launches (A/B)
// the slab sums of the two split-K launches live in their consumers (Sampling + KL forward / backward) instead of nt_slab_reduce_kernel
static bool latent_fuse_on() {
  const bool off = sv_knob_no_latent_fuse();
  return !off;
}
static bool latent_gemm_on(const sv_lgvae_plan* p) {
  static const bool off = SV_TUNE_FLAG("SV_NO_LATENT_GEMM");
  const bool off32 = sv_knob_no_latent_gemm_f32();       // (A/B: the fp32 forms of latent_gemm.hip)
  return !off && (p->d.dtype == SV_BF16 || !off32);
}

static double conv_flops(const sv_conv_desc& d) {
  return 2.0 * d.B * svg_oh(&d) * svg_ow(&d) * (double)d.Cout * d.KH * d.KW * d.Cin;
}

// FLOPs a POLYPHASE form of an upsample -> K x K conv layer really multiplies on the matrix pipe (real channels only; DESIGN.md section 5 "issued"):
//   main term: `taps` tap products per LOW-RES pixel where the direct form has 4 K^2 (per-class forms and the stride-2 input gradient: (5+4)^2 = 81 of 144 for
//   K = 6; the head's merged 25-tap form multiplies all 4 x 25 = 100 -- 19 of them structural zeros of the composite image -- of 144);
//   border terms: forward / weight gradient 2 (K-1) edge lines of H (W) hi-res pixels x K taps (poly_fix.hip, polyc_wgrad.hip's frame kernel); input gradient
//   four low-res edge lines x 4 strip rows x 9 taps (polyd_dgrad.hip).  Corner terms, the projection and the frame sum (< 1 % of a layer) are not counted.
static double poly_issued(const sv_conv_desc& d, int taps, bool dgrad) {
  const double main_ = conv_flops(d) * taps / (4.0 * d.KH * d.KW);
  const double border = 2.0 * d.B * (double)(d.H + d.W) * d.Cin * d.Cout * (dgrad ? 36.0 : (double)(d.KH - 1) * d.KH);
  return main_ + border;
}

// algorithmic HBM bytes of one conv-like launch (what a perfect kernel must move once): kind 0 forward (input [low-res when the
// resize is fused] + output + weights), 1 input gradient (dY + mask + dX), 2 weight gradient (input + dY + fp32 dW)
static double conv_bytes(const sv_conv_desc& d, int kind, size_t es) {
  const double in_px = (double)d.B * (d.ups_in ? d.H / 2 : d.H) * (d.ups_in ? d.W / 2 : d.W);
  const double out_px = (double)d.B * svg_oh(&d) * svg_ow(&d);
  const double w = (double)d.KH * d.KW * d.Cin * d.Cout;
  const double x = in_px * d.Cin * es, y = out_px * d.Cout * (d.y_f32 ? 4 : es);
  if (kind == 0) return x + y + w * es;
  if (kind == 1) return out_px * d.Cout * es + 2 * x + w * es;
  return x + out_px * d.Cout * es + w * 4;
}

#define SV_TRY(x)            \
  do {                       \
    int rc__ = (x);          \
    if (rc__) return rc__;   \
  } while (0)

// ---- the latent block on latent_gemm.hip: one builder per problem kind, one launch ladder; the im2col fall-backs stay with the callers
// out [M][ldo] = act(A [M][lda] . W^T + bias) gated by mask, W = the prepared image [N][ldw] at element w_off of the arena;
// S > 0: the K slices' fp32 slabs [S][M][ldo] instead (no bias / act / mask: their consumer applies them)
static NtGemmProb nt_prob(const sv_lgvae_plan* p, const void* A, int lda, int64_t w_off, int ldw, void* out, int ldo, int M, int N, int K,
                          const float* bias = nullptr, int act = SV_ACT_NONE, const void* mask = nullptr, int S = 0) {
  NtGemmProb g;
  memset(&g, 0, sizeof(g));
  g.f32 = p->d.dtype == SV_F32;
  g.A = A; g.lda = lda;
  g.W = (char*)p->buf(WARENA) + w_off * p->esz(); g.ldw = ldw;
  g.out = out; g.ldo = ldo;
  g.bias = bias; g.act = act; g.mask = mask;
  g.M = M; g.N = N; g.K = K;
  g.splitk = S > 0 ? S : 1; g.out_f32 = S > 0; g.slab_stride = S > 0 ? (int64_t)M * ldo : 0;
  return g;
}
static TnWgradProb tn_prob(const sv_lgvae_plan* p, const void* X, int ldx, const void* dY, int ldy, float* dW, float* dbias, int M, int Kw, int Kw_real, int N) {
  return TnWgradProb{X, ldx, dY, ldy, dW, dbias, M, Kw, Kw_real, N, p->d.dtype == SV_F32};
}
enum LatentRan { LAT_NOT_TAKEN, LAT_RAN, LAT_SLABS_LEFT };
// n <= 2 problems as one launch under the scope `name`.  LAT_NOT_TAKEN: nothing was launched and no scope booked (latent_gemm.hip is switched off or has no
// form for a problem): the caller's fall-back runs.  Slab problems are summed into sum_to[] right behind the launch (same scope), or with keep_slabs left
// unsummed for their consumer: LAT_SLABS_LEFT.
static int run_latent_nt(sv_lgvae_plan* p, const char* name, double fl, double by, NtGemmProb* q, int n, int bm, float* const* sum_to, bool keep_slabs,
                         hipStream_t st, LatentRan* ran) {
  *ran = LAT_NOT_TAKEN;
  if (!latent_gemm_on(p)) return SV_OK;
  for (int i = 0; i < n; ++i)
    if (!svk_nt_gemm_supported(q[i])) return SV_OK;
  Scope sc(p->prof, st, name, fl, by);
  const int rc = svk_nt_gemm_multi(q, n, bm, st);
  if (rc == SV_E_UNSUPPORTED) return SV_OK;
  if (rc) return rc;
  *ran = LAT_RAN;
  if (!q[0].out_f32) return SV_OK;
  if (!keep_slabs) return svk_nt_slab_reduce(q, sum_to, n, st);
  *ran = LAT_SLABS_LEFT;
  return SV_OK;
}
// the weight-gradient tile kernel: n <= 4 problems, whole batch per tile
static int run_latent_tn(sv_lgvae_plan* p, const char* name, double fl, double by, const TnWgradProb* q, int n, hipStream_t st, bool* taken) {
  *taken = false;
  if (!latent_gemm_on(p) || n > 4) return SV_OK;
  for (int i = 0; i < n; ++i)
    if (!svk_tn_wgrad_supported(q[i])) return SV_OK;
  Scope sc(p->prof, st, name, fl, by);
  *taken = true;
  return svk_tn_wgrad_multi(q, n, st);
}
// the memset a dz transition asks for (plan_latent.h).  GMVae has neither head pre-activations nor an x-hat network: its whole range is gz_x
static int zero_dz(sv_lgvae_plan* p, DzZero z, hipStream_t st) {
  if (z == DzZero::None) return SV_OK;
  if (z == DzZero::PreGz && !p->d.global_only) return p->bufs.zero(PRE, GZ_XH, st);
  return p->bufs.zero(GZ, GZ + p->ndec() - 1, st);
}

// The x and x-hat networks have twin layers of identical geometry: n of them go out as ONE launch
// (blockIdx.z picks the problem), which halves the per-launch fixed cost that dominates at B<=512.
struct FusedNll { const float* images6; void* grad[2]; float* part[2]; float gscale; int noout; };   // loss in the head's epilogue (tile_conv.hip)
static int run_fwd_layers(sv_lgvae_plan* p, int n, Layer* const* L, const void* const* x, const float* params,
                          void* const* y, hipStream_t st, const FusedNll* nll = nullptr) {
  TapGemmArgs a[2];
  double fl = 0, by = 0;
  for (int i = 0; i < n; ++i) {
    svg_fwd_args(&L[i]->d, &a[i]);
    a[i].A = x[i];
    a[i].Wt = (char*)p->buf(WARENA) + L[i]->wf_off * p->esz();
    a[i].bias = params + p->params[L[i]->bparam].off;
    a[i].out = y[i];
    if (nll) {
      a[i].nll_img = nll->images6; a[i].nll_ch = 3 * i; a[i].nll_grad = nll->grad[i]; a[i].nll_part = nll->part[i];
      a[i].nll_gscale = nll->gscale; a[i].nll_noout = nll->noout;
    }
    fl += conv_flops(L[i]->d);
    by += conv_bytes(L[i]->d, 0, p->esz());
  }
  if (!nll && L[0]->d.H == 1 && L[0]->d.W == 1 && L[0]->d.KH == 1 && !L[0]->d.y_f32) {   // Dense (d1): latent_gemm.hip
    NtGemmProb q[2];
    for (int i = 0; i < n; ++i) {
      const sv_conv_desc& d = L[i]->d;
      q[i] = nt_prob(p, x[i], d.ldx, L[i]->wf_off, svg_cin_pad(&d), y[i], d.ldy, d.B, d.Cout, d.Cin, a[i].bias, d.act);
    }
    LatentRan ran;
    SV_TRY(run_latent_nt(p, L[0]->sc_fwd.c_str(), fl, by, q, n, L[0]->d.B >= 256 ? 128 : 64, nullptr, false, st, &ran));
    if (ran != LAT_NOT_TAKEN) return SV_OK;
  }
  Scope sc(p->prof, st, L[0]->sc_fwd, fl, by);
  if (L[0]->polyc && !nll && n <= 2) {
    { double is = 0; for (int i = 0; i < n; ++i) is += poly_issued(L[i]->d, L[i]->d.KH == 6 ? 81 : 49, false); sc.issued(is); }
    // per-class polyphase (d4, d3): border kernel, then the four class problems of both networks in one launch
    const void* wf[2];
    const float* bs[2];
    for (int i = 0; i < n; ++i) { wf[i] = a[i].Wt; bs[i] = a[i].bias; }
    return svk_polyc_fwd_multi(&L[0]->d, n, x, wf, bs, y, p->pair(POLYCFIX), st);
  }
  if (svg_poly(&L[0]->d)) {
    { double is = 0; for (int i = 0; i < n; ++i) is += poly_issued(L[i]->d, 100, false); sc.issued(is); }
    // polyphase head: the out-of-image taps of the border rows / columns go to a workspace first; the conv's epilogue adds them
    const void* wfix[2];
    float* const* fixbuf = p->fpair(POLYFIX);
    const sv_conv_desc& d = L[0]->d;
    for (int i = 0; i < n; ++i) {
      wfix[i] = (const char*)p->buf(WARENA) + L[i]->wfix_off * p->esz();
      a[i].fix = fixbuf[i];
    }
    SV_TRY(svk_poly_fix_multi(n, x, wfix, nullptr, fixbuf, d.B, d.H / 2, d.W / 2, d.ldx, d.Cout, st, d.dtype));
  }
  return svk_conv_dispatch_multi(a, n, L[0]->d.dtype, svg_pick_cfg(L[0]->d.Cout), st);
}

// all parity classes of all n twin layers in one launch (stride 2: 4 classes x 2 networks = 8 problems)
static int run_dgrad_layers(sv_lgvae_plan* p, int n, Layer* const* L, const void* const* dy, const void* const* mask,
                            void* const* dx, bool f32_atomic, hipStream_t st, bool adj = false) {
  TapGemmArgs a[SV_MAX_MULTI];
  double fl = 0, by = 0;
  for (int i = 0; i < n; ++i) by += conv_bytes(L[i]->d, 1, p->esz());
  int m = 0, tap_cfg = svg_pick_cfg(L[0]->d.Cin);
  bool mixed = false;
  const int ncls = svg_dgrad_classes(&L[0]->d);
  if (!adj && !f32_atomic && ncls == 4) {              // classes that share one dY window (e2): one problem per network
    bool ok = true;
    for (int i = 0; i < n && ok; ++i) {
      ok = svg_dgrad_merged_args(&L[i]->d, &a[i]);
      a[i].A = dy[i]; a[i].Wt = (char*)p->buf(WARENA) + L[i]->wd_off[0] * p->esz(); a[i].out = dx[i]; a[i].mask = mask[i];
      fl += conv_flops(L[i]->d);
    }
    if (ok) {
      Scope sc(p->prof, st, L[0]->sc_dgrad, fl, by);
      const int rc = svk_conv_dispatch_multi(a, n, L[0]->d.dtype, svg_pick_cfg(a[0].N), st);
      if (rc != SV_E_UNSUPPORTED) return rc;
    }
    fl = 0;
  }
  for (int i = 0; i < n; ++i) {
    fl += conv_flops(L[i]->d);
    for (int c = 0; c < ncls; ++c, ++m) {
      uint8_t srctap[SV_MAX_TAPS];
      svg_dgrad_args(&L[i]->d, c, &a[m], srctap);
      a[m].A = dy[i];
      a[m].Wt = (char*)p->buf(WARENA) + L[i]->wd_off[c] * p->esz();
      a[m].out = dx[i];
      a[m].mask = mask[i];
      a[m].adj = adj ? 1 : 0;           // dx = the LOW-RES gradient, mask = the low-res activation (row_conv.hip)
      if (f32_atomic) {
        a[m].out_f32 = 1;
        a[m].accum = 1;
        int c2 = tap_cfg;
        a[m].splitk = svg_choose_splitk(a[m].M, a[m].N, (a[m].P + 7) / 8, &c2);
        if (m == 0) tap_cfg = c2;
        else if (c2 != tap_cfg) mixed = true;
      }
    }
  }
  if (adj) {                            // no fused kernel for this geometry: nothing was launched, the caller falls back
    if (!svk_row_conv_supported(a, m, L[0]->d.dtype)) return SV_E_UNSUPPORTED;
  }
  Scope sc(p->prof, st, L[0]->sc_dgrad, fl, by);
  if (mixed) {   // split-K problems whose widths pick different tiles: one launch each
    for (int i = 0; i < m; ++i) {
      int c2 = svg_pick_cfg(L[0]->d.Cin);
      a[i].splitk = svg_choose_splitk(a[i].M, a[i].N, (a[i].P + 7) / 8, &c2);
      SV_TRY(svk_conv_dispatch(a[i], L[0]->d.dtype, c2, st));
    }
    return SV_OK;
  }
  // the classes of a stride-2 layer have different tap counts but plan to the same tile grid
  return svk_conv_dispatch_multi(a, m, L[0]->d.dtype, tap_cfg, st);
}

static int run_wgrad_layers(sv_lgvae_plan* p, int n, Layer* const* L, const void* const* x, const void* const* dy,
                            float* grads, hipStream_t st) {
  WgradArgs a[SV_WGRAD_MAX_MULTI];
  double fl = 0, by = 0;
  for (int i = 0; i < n; ++i) by += conv_bytes(L[i]->d, 2, p->esz());
  const int64_t wsb = p->bbytes(WGRAD_WS) / (SV_WGRAD_MAX_MULTI * SideStreams::SIDE_MAX);   // one partial-sum slab region per stream and problem
  const std::string &ln = L[0]->ln, &nm = L[0]->sc_wgrad;
  // layers named in SV_WGRAD_MAIN keep their weight gradient on the main stream.  Measured (B = 512, 64x64): the side stream is
  // the critical path of the backward pass (it ends ~0.3 ms after the last input gradient), and d5's weight gradient slows the
  // concurrent d4 input gradient 2.5x; with d5 and the two tail layers e1, e2 on the main stream the step is 1.4 % shorter
  // ("" = everything on the side stream)
  // Batch dependence (re-measured per shard size): d5 on the main stream pays from ~768 images per launch (B = 512: -0.4 %)
  // and costs below that (B = 256: +0.6 %, 128: +4 %, 64: +2 %); e1 / e2 on the main stream pay at every size.
  // Round 3: d4's weight gradient on the rolling-window kernel (wgrad_roll.hip) is one persistent 8-wave workgroup per CU with the whole
  // register file: nothing co-resides with it, so beside the input-gradient chain it only gets the CUs that chain leaves (0.147 ms alone,
  // 0.27 live).  From 768 images per launch it stays on the main stream instead of d5's (re-measured, B = 512: "e1,e2,d5" 2.073 / 2.078 ms,
  // "e1,e2,d4" 2.056 / 2.063, "e1,e2,d5,d4" 2.072, "e1,e2,d4,d3" 2.076; B = 256 +-0, B = 128 / 64: +2.5 %, so not below the threshold)
  const char* const on_main_env = sv_knob_wgrad_main();
  const bool roll_off = sv_knob_no_wgrad_roll();
  const bool big = n * L[0]->d.B >= 768;
  // With TWO side streams (whole bf16 steps at this size, see run_phases) only the two tail layers stay: "e1,e2" 2.004 / 2.006 ms,
  // "e1,e2,d1" 2.008, "e1" / "e2" 2.03, "" 2.039, "e1,e2,d4" 2.061, "e1,e2,d5" 2.119.
  // fp32 (round 4, with the tile weight gradients: every launch is matrix-pipe-bound, two of them side by side only slow each other): the three
  // encoder layers on the main stream, the decoders' on the side stream -- "e1,e2,e3" 11.65-11.72 ms against "e1,e2,d5" 12.05-12.08, no side stream
  // at all 11.87, "e1,e2" 11.74, "e1" 11.80, "e1,e2,e3,d2" 11.77 (profiles/r04_f32_streams.txt)
  // (two side streams, re-measured with round 4's kernels: "e1" 1.643-1.647 ms, "e1,e2" 1.651-1.653, "e1,d1" 1.650-1.655, "e2" 1.668, "e1,e3" 1.663:
  //  profiles/r04_b512_streams.txt;
  //  512 images per launch, one side stream: "e1" 1.067-1.070 against 1.071-1.074 (profiles/r04_b256_sweep.txt); 256 and 128: "e1,e2" stays)
  const char* on_main = on_main_env ? on_main_env : !big ? (n * L[0]->d.B >= 512 ? "e1" : "e1,e2") : p->side.use >= 2 ? "e1" : (L[0]->d.dtype == SV_BF16 && !roll_off) ? "e1,e2,d4" :
                        L[0]->d.dtype == SV_F32 ? "e1,e2,e3" : "e1,e2,d5";
  if (strstr(on_main, ln.c_str())) p->side.slot = SideStreams::SIDE_MAX - 1;   // its own slab workspace: the side streams' slots are in use concurrently
  else st = p->side.wgrad_stream(st);
  if (L[0]->d.H == 1 && L[0]->d.W == 1 && L[0]->d.KH == 1 && n <= 4) {     // Dense (d1): latent_gemm.hip, whole batch per tile
    TnWgradProb q[4];
    double flq = 0;
    for (int i = 0; i < n; ++i) {
      const sv_conv_desc& d = L[i]->d;
      q[i] = tn_prob(p, x[i], d.ldx, dy[i], d.ldy, grads + p->params[L[i]->kparam].off, grads + p->params[L[i]->bparam].off, d.B, svg_cin_pad(&d), d.Cin, d.Cout);
      flq += conv_flops(d);
    }
    bool taken;
    SV_TRY(run_latent_tn(p, nm.c_str(), flq, by, q, n, st, &taken));
    if (taken) return SV_OK;
  }
  // the decoder head's weight gradient in polyphase form (poly_wgrad.hip) from ~768 images per launch (its three small
  // kernels cost more than they save below that: 16 images 42 vs 20 us; 1024 images 132 vs 184 us)
  static const bool no_pw = SV_TUNE_FLAG("SV_NO_POLY_WGRAD");
  // (round 2, tile-kernel main term: 512 images per launch +0.4 %, 1024 -1.0 % -> 768; round 4, rolling-window main term (wgrad_p5.hip): 512 images per
  //  launch -0.7 %, 256 +2.5 % -> 512: profiles/r04_poly_wgrad_min_sweep.txt)
  static const int pw_min = SV_TUNE_INT("SV_POLY_WGRAD_MIN", 512);
  if (!no_pw && L[0]->d.dtype == SV_BF16 && svg_poly(&L[0]->d) && n * L[0]->d.B >= pw_min && n <= 2 &&
      svk_poly_wgrad_supported(L[0]->d.H / 2, L[0]->d.W / 2, svg_cin_pad(&L[0]->d), L[0]->d.Cout)) {   // else: the direct form below
    float* const* pw = p->fpair(POLYW);
    float *dwv[2], *dbv[2];
    const int Cin = svg_cin_pad(&L[0]->d);
    for (int i = 0; i < n; ++i) {
      svg_poly_wgrad_args(&L[i]->d, &a[i]);
      a[i].A = x[i]; a[i].dY = dy[i]; a[i].dW = pw[i]; a[i].dbias = pw[i] + 25 * Cin * 32;
      a[i].ws = (float*)((char*)p->buf(WGRAD_WS) + (p->side.slot * SV_WGRAD_MAX_MULTI + i) * wsb); a[i].ws_bytes = wsb;
      dwv[i] = grads + p->params[L[i]->kparam].off; dbv[i] = grads + p->params[L[i]->bparam].off;
      fl += conv_flops(L[i]->d);
    }
    Scope sc(p->prof, st, nm, fl, by);
    { double is = 0; for (int i = 0; i < n; ++i) is += poly_issued(L[i]->d, 100, false); sc.issued(is); }
    SV_TRY(svk_wgrad_bf16_forms_multi(a, n, st));        // wgrad_p5 or wgrad_tile
    const sv_conv_desc& d = L[0]->d;
    return svk_poly_wgrad_finish(n, x, dy, pw, dwv, dbv, d.B, d.H / 2, d.W / 2, d.ldx, Cin, d.Cout, SV_POLY_WGRAD_NWG, st);
  }
  // fp32: the polyphase weight gradient of the upsample -> conv layers (polyc_wgrad.hip: d4 per parity class, the head merged)
  static const int pcw_min = SV_TUNE_INT("SV_POLYC_WGRAD_MIN", 0);
  if (L[0]->d.dtype == SV_F32 && n <= 2 && n * L[0]->d.B >= pcw_min && svg_polyc_wgrad_form(&L[0]->d) && L[0]->polycw >= 0 &&
      !(p->polycw_bad >> L[0]->polycw & 1) && p->bufs.has(L[0]->polycw)) {       // (has: the one workspace a plan may lack by its shapes, see LGVAE_BUFFERS)
    float *dwv[2], *dbv[2], *slab[2];
    for (int i = 0; i < n; ++i) {
      dwv[i] = grads + p->params[L[i]->kparam].off; dbv[i] = grads + p->params[L[i]->bparam].off;
      slab[i] = (float*)((char*)p->buf(WGRAD_WS) + (p->side.slot * SV_WGRAD_MAX_MULTI + i) * wsb);
      fl += conv_flops(L[i]->d);
    }
    Scope sc(p->prof, st, nm, fl, by);
    { double is = 0; for (int i = 0; i < n; ++i) is += poly_issued(L[i]->d, svg_polyc_wgrad_form(&L[i]->d) == 2 ? 100 : 81, false); sc.issued(is); }
    const int rc = svk_polyc_wgrad_multi(&L[0]->d, n, x, dy, dwv, dbv, slab, wsb, p->fpair(L[0]->polycw), st);
    if (rc != SV_E_UNSUPPORTED) return rc;
    p->polycw_bad |= 1u << L[0]->polycw;
    fl = 0;
  }
  // (every layer reduces its own slabs on its own stream.  One reduce for all layers after the join was measured and removed: profiles/r03_f_defer.txt,
  // the slabs are then read cold from HBM on the critical path -- B = 512 -0.5..1 %, B = 64 +5 %)
  for (int i = 0; i < n; ++i) {
    svg_wgrad_args(&L[i]->d, &a[i]);
    a[i].A = x[i]; a[i].dY = dy[i];
    a[i].dW = grads + p->params[L[i]->kparam].off;
    a[i].dbias = grads + p->params[L[i]->bparam].off;
    a[i].ws = (float*)((char*)p->buf(WGRAD_WS) + (p->side.slot * SV_WGRAD_MAX_MULTI + i) * wsb); a[i].ws_bytes = wsb;
    fl += conv_flops(L[i]->d);
  }
  Scope sc(p->prof, st, nm, fl, by);
  sc.issued(fl);                        // (a polyphase form above may have been refused after booking its count)
  sc.split(L[0]->sc_reduce, 0, a[0].ev_mid);
  return svk_wgrad_dispatch_multi(a, n, L[0]->d.dtype, svg_pick_cfg(L[0]->d.Cout), st);
}

// early: side stream 0 (SideStreams::early_stream) or nullptr -- the decoders' half of the job table goes there, the encoders' half stays in front of their forward
static int phase_prep(sv_lgvae_plan* p, const sv_lgvae_step_args* s, hipStream_t st, hipStream_t early) {
  Scope sc(p->prof, st, "prep_weights", 0, (double)p->nparams * (4 + 2.0 * p->esz()));
  const PrepJob* jobs = (const PrepJob*)p->buf(JOBS);
  if (!early || p->dec_block0 == 0) return svk_prep_weights(s->params, p->buf(WARENA), p->d.dtype, jobs, (int)p->jobs.size(), p->prep_blocks, st);
  SV_TRY(svk_prep_weights(s->params, p->buf(WARENA), p->d.dtype, jobs, (int)p->jobs.size(), p->prep_blocks - p->dec_block0, early, p->dec_block0));
  return svk_prep_weights(s->params, p->buf(WARENA), p->d.dtype, jobs, (int)p->jobs.size(), p->dec_block0, st);
}

static int phase_forward(sv_lgvae_plan* p, const sv_lgvae_step_args* s, bool do_enc, bool do_dec, hipStream_t st,
                         bool want_nll = false) {
  p->nll_fused = false;
  const sv_lgvae_desc& d = p->d;
  const int B = d.B, H = d.H, W = d.W, dt = d.dtype;
  const int Lg = d.global_latent, Ll = d.local_latent, Lc = Lg + Ll;
  const bool no_twin = no_twin_pointwise();
  LatentBlock& lat = p->lat;
  bool pre_slabs = false;
  const int nd = p->ndec();
  if (do_enc) {
    // the head pre-activations (split-K partial sums) and dz (split-K dgrad of d1) accumulate with atomics: zeroed here -- not needed once both split-K launches
    // of this plan have gone through latent_gemm.hip's slabs (nothing accumulates into these buffers, and the backward must not re-zero dz either).
    // GMVae: the caller's encoder_x is the only encoder -- this phase zeroes dz (split-K target of d1's input gradient) and fills in8_x
    const bool slab_path = !d.global_only && latent_gemm_on(p) && lat.head_ok && lat.d1_ok && !d.external_global_encoder;
    const DzStep t = dz_transition(lat.dz, DzEvent::EncFwd, slab_path);
    SV_TRY(zero_dz(p, t.zero, st));
    lat.dz = t.next;
  }
  if (do_enc && !(s->phases & SV_PHASE_INPUTS_STAGED)) {      // (staged: sv_scramble_gather_staged filled in8_x / in8_xh for this images6)
    Scope sc(p->prof, st, "split_pad", 0, (double)B * H * W * (24 + 16.0 * p->esz()));
    SV_TRY(svk_split_pad(s->images6, p->buf(IN8, 0), p->buf(IN8, 1), dt, (int64_t)B * H * W, st));
  }
  if (d.global_only) do_enc = false;           // (that was all of the encoders' phase: the plan has none)
  if (do_enc) {
    static const BufId in_id[3] = {IN8, A1, A2}, out_id[3] = {A1, A2, A3};
    for (int l = 0; l < 3; ++l) {
      Layer* Ls[2] = {&p->enc[0][l], &p->enc[1][l]};
      const int e0 = d.external_global_encoder ? 1 : 0;     // SPLIT-GMVAE: the caller runs its own encoder_x
      SV_TRY(run_fwd_layers(p, 2 - e0, Ls + e0, p->pair(in_id[l]) + e0, s->params, p->pair(out_id[l]) + e0, st));
    }
  }
  if (do_enc) {
    // heads: split-K GEMMs into the zeroed fp32 pre-activations (bias + softplus live in reparam_kl_fwd); the two
    // networks' heads share one launch (each alone is 16 output tiles)
    const int e0 = d.external_global_encoder ? 1 : 0;
    TapGemmArgs a[2];
    int cfg = 0, cfgs[2] = {0, 0};
    double fl = 0, by = 0;
    for (int e = e0; e < 2; ++e) {
      Layer& Lh = p->enc[e][3];
      TapGemmArgs& t = a[e - e0];
      svg_fwd_args(&Lh.d, &t);
      t.A = p->buf(A3, e);
      t.Wt = (char*)p->buf(WARENA) + Lh.wf_off * p->esz();
      t.bias = nullptr; t.out = p->buf(PRE, e); t.out_f32 = 1;
      cfg = svg_pick_cfg(Lh.d.Cout);
      t.splitk = svg_choose_splitk(t.M, t.N, (t.P + 7) / 8, &cfg);
      cfgs[e - e0] = cfg;
      fl += conv_flops(Lh.d);
      by += conv_bytes(Lh.d, 0, p->esz());
    }
    NtGemmProb q[2];
    float* outs[2];
    for (int e = e0; e < 2; ++e) {
      const sv_conv_desc& hd = p->enc[e][3].d;
      q[e - e0] = nt_prob(p, p->buf(A3, e), hd.Cin, p->enc[e][3].wf_off, hd.Cin, p->buf(LAT_WS, e), hd.Cout, B, hd.Cout, hd.Cin, nullptr, SV_ACT_NONE, nullptr, lat.head_S[e]);
      outs[e - e0] = (float*)p->buf(PRE, e);
    }
    // Sampling + KL sum the slabs themselves, in slice order: the same bits (more than 16 slices: one wave per row reads them too slowly, B = 64: +4 %)
    const bool fuse = latent_fuse_on() && !e0 && !no_twin && lat.head_S[0] <= 16 && lat.head_S[1] <= 16;
    LatentRan ran;
    SV_TRY(run_latent_nt(p, "fwd.head", fl, by, q, 2 - e0, 64, outs, fuse, st, &ran));
    if (ran != LAT_NOT_TAKEN) lat.head_ok = true;
    pre_slabs = ran == LAT_SLABS_LEFT;
    if (ran == LAT_NOT_TAKEN) {
      Scope sc(p->prof, st, "fwd.head", fl, by);
      if (e0 || cfgs[0] == cfgs[1]) SV_TRY(svk_tap_gemm_multi(a, 2 - e0, dt, cfgs[0], st));
      else
        for (int e = 0; e < 2; ++e) SV_TRY(svk_tap_gemm(a[e], dt, cfgs[e], st));   // latent sizes with different tiles
    }
  }
  if (do_enc) {
    // Sampling + KL: both networks in one launch; one network per launch for SPLIT-GMVAE (the caller's encoder is the x network) and under SV_NO_TWIN_POINTWISE
    const int e0 = d.external_global_encoder ? 1 : 0, per = no_twin ? 1 : 2 - e0;
    ReparamFwdArgs a[2];
    for (int e = e0; e < 2; ++e) {
      const Layer& Lh = p->enc[e][3];
      // mean bias and sd bias are separate Keras tensors
      a[e] = {(const float*)p->buf(pre_slabs ? LAT_WS : PRE, e), s->params + p->params[Lh.kparam + 1].off, s->params + p->params[Lh.kparam + 3].off,
              e == 0 ? s->eps_x : s->eps_x_hat, (float*)p->buf(EPS, e), (float*)p->buf(Z_MEAN, e), (float*)p->buf(Z_SIG, e), (float*)p->buf(Z, e),
              p->buf(ZCAT), (float*)p->buf(KL, e), Lc, e == 0 ? 0 : Lg, e == 0 ? Lg : Ll, e, pre_slabs ? lat.head_S[e] : 0, pre_slabs ? lat.head_stride[e] : 0};
    }
    for (int e = e0; e < 2; e += per) {
      Scope sc(p->prof, st, "reparam_kl_fwd", 0, (double)B * (per == 2 ? Lg + Ll : a[e].L) * 16);
      SV_TRY(svk_reparam_kl_fwd(a + e, per, dt, B, s->seed, s->step, s->sample_offset, st, p->dyn));
    }
  }
  if (do_dec) {
    SV_TRY(p->side.early_wait(st));               // the decoders' weight images (and the zeroed gradient buffer) of this call's early side work
    const void* zin[2] = {p->buf(ZCAT), (const char*)p->buf(ZCAT) + (size_t)Lg * p->esz()};
    {   // d1 differs between the twins (zcat vs local-only input): two shapes, one launch
      Layer* Ls[2] = {&p->dec[0][0], &p->dec[1][0]};
      SV_TRY(run_fwd_layers(p, nd, Ls, zin, s->params, p->pair(H1), st));
    }
    {
      Layer* Ls[2] = {&p->dec[0][1], &p->dec[1][1]};
      SV_TRY(run_fwd_layers(p, nd, Ls, p->pair(H1), s->params, p->pair(H2), st));
    }
    // d3..d5 consume the 2x bilinear upsample of the previous activation (vae/model.py:163-167).
    // Fused (bf16): the conv/wgrad tile staging interpolates from the low-res tensor, u2/u3/u4 are
    // never written.  Materialised (fp32 parity path, whose wgrad runs on the im2col kernel).
    static const BufId lo_id[3] = {H2, H3, H4}, hi_id[3] = {U2, U3, U4}, out_id[3] = {H3, H4, OUT6};
    for (int l = 0; l < 3; ++l) {
      Layer* Ls[2] = {&p->dec[0][2 + l], &p->dec[1][2 + l]};
      const void* xs[2] = {nullptr, nullptr};
      const BufPair ys = p->pair(out_id[l]);
      for (int k = 0; k < nd; ++k) {
        xs[k] = p->buf(lo_id[l], k);
        if (!Ls[k]->d.ups_in) {
          Scope sc(p->prof, st, "upsample_fwd", 0, 0);
          SV_TRY(sv_upsample2x_fwd(xs[k], p->buf(hi_id[l], k), dt, B, Ls[k]->d.H / 2, Ls[k]->d.W / 2, Ls[k]->d.Cin, st));
          xs[k] = p->buf(hi_id[l], k);
        }
      }
      if (l == 2 && want_nll && svg_poly(&Ls[0]->d) && d.H * d.W >= 1024) {
        // training step: the head's epilogue evaluates the loss of its own pixels (NLL partial sums + the gradient record
        // g5), so dlogistic_kernel and its re-read of out6 drop out of the step (phase_loss then only sums the partials)
        FusedNll f;
        f.images6 = s->images6; f.gscale = 1.0f / (float)d.B; f.noout = (s->phases & SV_PHASE_NO_RECON) ? 1 : 0;
        for (int k = 0; k < 2; ++k) { f.grad[k] = p->buf(G5, k); f.part[k] = (float*)p->buf(NLLPART, k); }
        const int rc = run_fwd_layers(p, nd, Ls, xs, s->params, ys, st, &f);
        if (rc == SV_OK) { p->nll_fused = true; continue; }
        if (rc != SV_E_UNSUPPORTED) return rc;
      }
      SV_TRY(run_fwd_layers(p, nd, Ls, xs, s->params, ys, st));
    }
  }
  return SV_OK;
}

static int phase_loss(sv_lgvae_plan* p, const sv_lgvae_step_args* s, bool with_grad, hipStream_t st) {
  const sv_lgvae_desc& d = p->d;
  const bool from_parts = p->nll_fused && with_grad;   // the head's epilogue left per-tile NLL sums and g5 (phase_forward): finalize_losses
                                                       // forms the per-image sums itself (fixed order), no separate kernel
  if (!from_parts) {
    // algorithmic bytes: read x, m, log_scale (12 B/element) + write dm, dls (2 * esz B/element); both networks
    Scope sc(p->prof, st, "dlogistic_nll", 0, p->ndec() * d.B * d.H * d.W * 3.0 * (12.0 + (with_grad ? 2.0 * p->esz() : 0.0)));
    auto zs = [&](int id, int64_t esz) {               // elements from the x network's record to the x-hat network's
      if (d.global_only) return (int64_t)0;            // (one network: no second record)
      return (int64_t)((char*)p->buf(id, 1) - (char*)p->buf(id, 0)) / esz;
    };
    SV_TRY(svk_dlogistic_nll_multi(s->images6, 0, (const float*)p->buf(OUT6), zs(OUT6, 4), (float*)p->buf(NLL), zs(NLL, 4),
                                   with_grad ? p->buf(G5) : nullptr, zs(G5, (int64_t)p->esz()), d.dtype, 1.0f / (float)d.B, d.B, d.H, d.W,
                                   (float*)p->buf(NLLPART), zs(NLLPART, 4), p->ndec(), st));
  }
  const int HWp = d.H * d.W;
  // NULL ON PURPOSE (global_only, see LGVAE_BUFFERS): the plan has no x-hat network and no KL buffers -- finalize_losses reads those terms as zero
  SV_TRY(svk_finalize_losses((const float*)p->buf(NLL, 0), (const float*)p->buf(NLL, 1), (const float*)p->buf(KL, 0), (const float*)p->buf(KL, 1), d.B, d.beta,
                             (float*)p->buf(LOSSES), (float*)p->buf(METRIC_ACC), s->accumulate_metrics, st,
                             from_parts ? (const float*)p->buf(NLLPART, 0) : nullptr, from_parts ? (const float*)p->buf(NLLPART, 1) : nullptr,
                             HWp > 1024 ? HWp / 1024 : 1));
  return SV_OK;
}

static int phase_bwd_decoders(sv_lgvae_plan* p, const sv_lgvae_step_args* s, hipStream_t st) {
  const int nd = p->ndec();
  // What every decoders' backward needs before it starts (a second backward over the same forward: re-zero the split-K dz accumulators); how d1's input
  // gradient leaves dz is known only at the end of the phase, where the transition that really happened is applied
  LatentBlock& lat = p->lat;
  const DzState dz_in = lat.dz;
  // (t_in.zero is the zero of EVERY decoders'-backward transition out of dz_in, with one exception: Stale + accumulating, handled at d1 below -- see
  //  dz_transition: DecBwdSlabs and DecBwdGz return the same `used ? Gz : None` but for that case.  So issuing t_in.zero here and the difference there
  //  is the zero of the one transition that really happens, and both memsets precede the only writer of gz_*)
  const DzStep t_in = dz_transition(dz_in, DzEvent::DecBwdSlabs, true);
  SV_TRY(zero_dz(p, t_in.zero, st));
  lat.dz = t_in.next;                  // (an error return below leaves a state that re-zeroes, as the memset above is spent)
  const sv_lgvae_desc& d = p->d;
  const int B = d.B, H = d.H, W = d.W, dt = d.dtype;
  const int Lg = d.global_latent;
  const void* none[2] = {nullptr, nullptr};
  static const BufId gy_id[3] = {G5, G4, G3};       // gradient at the layer output
  static const BufId gu_id[3] = {GU4, GU3, GU2};    // gradient at the (virtual) upsampled input
  static const BufId lo_id[3] = {H4, H3, H2};       // low-res activation feeding the upsample
  static const BufId hi_id[3] = {U4, U3, U2};
  static const BufId gl_id[3] = {G4, G3, G2};       // gradient at the low-res activation
  static const char* const ups_scope[3] = {"upsample_bwd.4", "upsample_bwd.3", "upsample_bwd.2"};
  for (int l = 0; l < 3; ++l) {                                // d5, d4, d3
    const int li = 4 - l;
    Layer* Ls[2] = {&p->dec[0][li], &p->dec[1][li]};
    const BufPair gy = p->pair(gy_id[l]), gu = p->pair(gu_id[l]), lo = p->pair(lo_id[l]), gl = p->pair(gl_id[l]);
    const void* xin[2] = {nullptr, nullptr};
    for (int k = 0; k < nd; ++k) xin[k] = p->buf(Ls[k]->d.ups_in ? lo_id[l] : hi_id[l], k);
    SV_TRY(run_wgrad_layers(p, nd, Ls, xin, gy, s->grads, st));
    // the input gradient lands at the LOW-RES activation in one launch where the fused kernel exists (ResizeBilinearGrad +
    // ReluGrad in the epilogue of Conv2DBackpropInput: the hi-res gradient gu never reaches HBM) ...
    // (it works on whole images -- its low-res rows straddle row bands -- so below ~one image per workgroup slot the banded
    // plain input gradient + upsample2x_bwd is faster: 64 images per network d5 43 vs 55 us, d4 40 vs 49; 128: 69 vs 56)
    static const bool no_adj = SV_TUNE_FLAG("SV_NO_FUSED_ADJOINT");
    // (round 4, with the adjoint of d3 / d4 on the matrix pipe: 128 images per launch -- config 4's 64-image shard -- 0.641 -> 0.631 ms fused; the
    //  default moved from 256 to 128)
    static const int adj_min = SV_TUNE_INT("SV_RC_ADJ_MIN", 128);
    int frc = SV_E_UNSUPPORTED;
    if (Ls[0]->polyd && (nd == 1 || Ls[1]->polyd)) {
      // fp32: the polyphase form (polyd_dgrad.hip): conv-transpose + resize adjoint + ReLU gate as one stride-2 conv over dY, edge terms through a workspace
      const void* wp[2];
      double fl = 0, by = 0;
      for (int k = 0; k < nd; ++k) {
        wp[k] = (const char*)p->buf(WARENA) + Ls[k]->wd_off[0] * p->esz();
        fl += conv_flops(Ls[k]->d); by += conv_bytes(Ls[k]->d, 1, p->esz());
      }
      Scope sc(p->prof, st, Ls[0]->sc_dgrad, fl, by);
      { double is = 0; for (int k = 0; k < nd; ++k) is += poly_issued(Ls[k]->d, 81, true); sc.issued(is); }
      frc = svk_polyd_dgrad_multi(&Ls[0]->d, nd, gy, wp, lo, gl, p->pair(POLYD), st);
    }
    if (frc == SV_E_UNSUPPORTED && Ls[0]->d.ups_in && (nd == 1 || Ls[1]->d.ups_in) && !no_adj && nd * B >= adj_min)
      frc = run_dgrad_layers(p, nd, Ls, gy, lo, gl, false, st, true);
    if (frc != SV_E_UNSUPPORTED) { SV_TRY(frc); continue; }
    // ... else the hi-res gradient goes through HBM and a stand-alone adjoint pass
    SV_TRY(run_dgrad_layers(p, nd, Ls, gy, none, gu, false, st));
    {
      const int h = (H / 2) >> l, w = (W / 2) >> l, c = 32 << l;
      const int64_t lo_bytes = (int64_t)B * h * w * c * p->esz();
      const bool contig = nd == 2 && (const char*)gu[1] == (const char*)gu[0] + 4 * lo_bytes &&
                          (const char*)lo[1] == (const char*)lo[0] + lo_bytes && (const char*)gl[1] == (const char*)gl[0] + lo_bytes;
      Scope sc(p->prof, st, ups_scope[l], 0, nd * 6.0 * lo_bytes);   // read g_hi (4x) + mask, write g_lo; both networks
      if (contig) SV_TRY(sv_upsample2x_bwd(gu[0], lo[0], gl[0], dt, 2 * B, h, w, c, st));
      else
        for (int k = 0; k < nd; ++k) SV_TRY(sv_upsample2x_bwd(gu[k], lo[k], gl[k], dt, B, h, w, c, st));
    }
  }
  {
    // d2 (input h1 = relu(d1): mask fused in the dgrad epilogue)
    Layer* Ls[2] = {&p->dec[0][1], &p->dec[1][1]};
    SV_TRY(run_wgrad_layers(p, nd, Ls, p->pair(H1), p->pair(G2), s->grads, st));
    SV_TRY(run_dgrad_layers(p, nd, Ls, p->pair(G2), p->pair(H1), p->pair(G1), false, st));
  }
  {
    // d1 (dense): dz accumulated in fp32 over split K; the twins (different input widths) share the launches
    Layer Ld[2] = {p->dec[0][0], p->dec[1][0]};
    Layer* Ls[2] = {&p->dec[0][0], &p->dec[1][0]};
    Layer* Lds[2] = {&Ld[0], &Ld[1]};
    const void* zin[2] = {p->buf(ZCAT), (const char*)p->buf(ZCAT) + (size_t)Lg * p->esz()};
    const BufPair g1 = p->pair(G1), gz = p->pair(GZ);
    SV_TRY(run_wgrad_layers(p, nd, Ls, zin, g1, s->grads, st));
    for (int k = 0; k < nd; ++k) Ld[k].d.ldx = Ld[k].d.Cin;   // dz has its own row pitch (Lz), not the zcat pitch
    NtGemmProb q[2];
    float* outs[2];
    double fl = 0, by = 0;
    for (int k = 0; k < nd; ++k) {
      const sv_conv_desc& dd = Ld[k].d;
      q[k] = nt_prob(p, g1[k], dd.ldy, Ld[k].wd_off[0], svg_gdy(&dd), p->buf(LAT_WS, k), dd.Cin, B, dd.Cin, dd.Cout, nullptr, SV_ACT_NONE, nullptr, lat.d1_S[k]);
      outs[k] = (float*)gz[k];
      fl += conv_flops(dd); by += conv_bytes(dd, 1, p->esz());
    }
    // reparam_kl_bwd sums the slabs (SPLIT-GMVAE and GMVae read gz_x: summed here)
    const bool fuse = latent_fuse_on() && !d.external_global_encoder && !no_twin_pointwise() && lat.d1_S[0] <= 16 && lat.d1_S[1] <= 16;
    LatentRan ran;
    SV_TRY(run_latent_nt(p, "dgrad.d1", fl, by, q, nd, 64, outs, fuse, st, &ran));
    if (ran != LAT_NOT_TAKEN) lat.d1_ok = true;
    if (ran != LAT_SLABS_LEFT) {       // (slabs left: lat.dz is t_in.next already)
      // dz in gz_*: summed from the slabs (which overwrites gz_*), or accumulated by the im2col kernel's split-K atomics into a gz_* that must be zero --
      // after a forward that skipped the zero fill (DzState::Stale; no current shape reaches this fall-back) it is zeroed here
      const DzStep t = dz_transition(dz_in, DzEvent::DecBwdGz, ran == LAT_RAN);
      if (t.zero != t_in.zero) SV_TRY(zero_dz(p, t.zero, st));
      lat.dz = t.next;
      if (ran == LAT_NOT_TAKEN) SV_TRY(run_dgrad_layers(p, nd, Lds, g1, none, gz, true, st));
    }
  }
  return SV_OK;
}

static int phase_bwd_encoders(sv_lgvae_plan* p, const sv_lgvae_step_args* s, bool do_heads, bool do_convs, hipStream_t st, bool buckets = false) {
  const sv_lgvae_desc& d = p->d;
  const int B = d.B, dt = d.dtype;
  const int Lg = d.global_latent, Ll = d.local_latent, Lc = Lg + Ll;
  const float kl_scale = d.beta / (float)B;
  const int e0 = d.external_global_encoder ? 1 : 0;
  if (d.global_only) return SV_OK;            // GMVae: the only encoder is the caller's (it reads dL/dz_x from gz_x)
  LatentBlock& lat = p->lat;
  if (do_heads) {                             // (KL terms only -- no decoder backward since a forward that skipped the zero fill: dz = 0)
    const DzStep t = dz_transition(lat.dz, DzEvent::EncHeadBwd, false);
    SV_TRY(zero_dz(p, t.zero, st));
    lat.dz = t.next;
  }
  if (do_heads) {
    // the adjoint of Sampling + KL, launched as the forward is (phase_forward).  decoder_x's dz is [B, Lc]: columns [0, Lg) belong to z_x, [Lg, Lc) to z_x-hat,
    // which also gets decoder_x-hat's dz.  DzState::InSlabs (twin launch only): the K-slice slabs of d1's input gradient instead, summed in the kernel
    Scope sc(p->prof, st, "reparam_kl_bwd", 0, 0);
    const bool slabs = lat.dz == DzState::InSlabs;
    const int per = no_twin_pointwise() ? 1 : 2 - e0, src = slabs ? LAT_WS : GZ;
    const int S0 = slabs ? lat.d1_S[0] : 0, S1 = slabs ? lat.d1_S[1] : 0;
    const int64_t sd0 = slabs ? lat.d1_stride[0] : 0, sd1 = slabs ? lat.d1_stride[1] : 0;
    const float* dzx = (const float*)p->buf(src, 0);
    const ReparamBwdArgs a[2] = {
        {dzx, nullptr, (const float*)p->buf(Z_MEAN, 0), (const float*)p->buf(Z_SIG, 0), (const float*)p->buf(EPS, 0), p->buf(GHEAD, 0), Lc, 0, Lg, S0, 0, sd0, 0},
        {dzx + Lg, (const float*)p->buf(src, 1), (const float*)p->buf(Z_MEAN, 1), (const float*)p->buf(Z_SIG, 1), (const float*)p->buf(EPS, 1), p->buf(GHEAD, 1),
         Lc, Ll, Ll, S0, S1, sd0, sd1}};
    for (int e = e0; e < 2; e += per) SV_TRY(svk_reparam_kl_bwd(a + e, per, kl_scale, dt, B, st));
  }
  if (do_heads) {
    // heads: two Keras kernels/biases per network -> wgrad problems on the column halves of ghead, all in one launch
    WgradArgs a[4];
    int n = 0;
    double fl = 0, by = 0;
    for (int e = e0; e < 2; ++e) by += conv_bytes(p->enc[e][3].d, 2, p->esz());
    for (int e = e0; e < 2; ++e) {
      Layer* L = p->enc[e];
      const int Lh = e == 0 ? Lg : Ll;
      for (int h = 0; h < 2; ++h, ++n) {
        svg_wgrad_args(&L[3].d, &a[n]);
        a[n].A = p->buf(A3, e);
        a[n].dY = (const char*)p->buf(GHEAD, e) + (size_t)h * Lh * p->esz();
        a[n].ycols = Lh; a[n].N = Lh;
        a[n].dW = s->grads + p->params[L[3].kparam + 2 * h].off;
        a[n].dbias = s->grads + p->params[L[3].kparam + 2 * h + 1].off;
        fl += conv_flops(L[3].d) / 2;
      }
    }
    {
      hipStream_t ws = p->side.wgrad_stream(st);
      TnWgradProb q[4];
      for (int i = 0; i < n; ++i) q[i] = tn_prob(p, a[i].A, a[i].lda, a[i].dY, a[i].ldy, a[i].dW, a[i].dbias, B, a[i].Cin_pad, a[i].Cin_real, a[i].N);
      bool taken;
      SV_TRY(run_latent_tn(p, "wgrad.head", fl, by, q, n, ws, &taken));
      if (!taken) {
        Scope sc(p->prof, ws, "wgrad.head", fl, by);
        const int cg = svg_pick_cfg(Lg), cl = svg_pick_cfg(Ll);      // the narrower tile serves both widths
        SV_TRY(svk_wgrad_dispatch_multi(a, n, dt, e0 ? cl : (cg > cl ? cg : cl), ws));
      }
    }
    Layer* Ls[2] = {&p->enc[0][3], &p->enc[1][3]};
    const BufPair gh = p->pair(GHEAD), a3 = p->pair(A3), ga3 = p->pair(GA3);
    NtGemmProb q[2];
    double flh = 0, byh = 0;
    for (int e = e0; e < 2; ++e) {
      const sv_conv_desc& hd = p->enc[e][3].d;
      q[e - e0] = nt_prob(p, gh[e], hd.Cout, p->enc[e][3].wd_off[0], hd.Cout, ga3[e], hd.Cin, B, hd.Cin, hd.Cout, nullptr, SV_ACT_NONE, a3[e]);
      flh += conv_flops(hd); byh += conv_bytes(hd, 1, p->esz());
    }
    LatentRan ran;
    SV_TRY(run_latent_nt(p, "dgrad.head", flh, byh, q, 2 - e0, B >= 256 ? 128 : 64, nullptr, false, st, &ran));
    if (ran == LAT_NOT_TAKEN) SV_TRY(run_dgrad_layers(p, 2 - e0, Ls + e0, gh + e0, a3 + e0, ga3 + e0, false, st));
    if (buckets) SV_TRY(p->side.record_bucket(1, st));       // the heads' weight gradients are enqueued (main or side stream)
  }
  if (do_convs) {
    static const BufId act_id[3] = {IN8, A1, A2}, g_id[3] = {GA1, GA2, GA3};
    for (int l = 2; l >= 0; --l) {
      Layer* Ls[2] = {&p->enc[0][l], &p->enc[1][l]};
      const BufPair x = p->pair(act_id[l]), gy = p->pair(g_id[l]);
      SV_TRY(run_wgrad_layers(p, 2 - e0, Ls + e0, x + e0, gy + e0, s->grads, st));
      if (l == 0) break;
      SV_TRY(run_dgrad_layers(p, 2 - e0, Ls + e0, gy + e0, x + e0, p->pair(g_id[l - 1]) + e0, false, st));
    }
    if (buckets) SV_TRY(p->side.record_bucket(2, st));
  }
  return SV_OK;
}

}  // namespace

extern "C" int64_t sv_lgvae_param_count(const sv_lgvae_desc* d) {
  if (check_desc(d) != SV_OK) return -1;
  auto v = build_params(d);
  return v.back().off + (v.back().count + 3) / 4 * 4;
}

extern "C" int sv_lgvae_param_info(const sv_lgvae_desc* d, int32_t index, int64_t* offset, int32_t* ndim,
                                   int64_t shape[4], char name[96]) {
  int rc = check_desc(d);
  if (rc) return rc;
  auto v = build_params(d);
  if (index < 0 || index >= (int)v.size()) return SV_E_BADARG;
  const ParamInfo& p = v[index];
  if (offset) *offset = p.off;
  if (ndim) *ndim = p.ndim;
  if (shape) for (int i = 0; i < 4; ++i) shape[i] = p.shape[i];
  if (name) snprintf(name, 96, "%s", p.name.c_str());
  return SV_OK;
}

extern "C" int sv_lgvae_plan_create(const sv_lgvae_desc* d, sv_lgvae_plan** out) {
  int rc = check_desc(d);
  if (rc) return rc;
  if (!out) return SV_E_BADARG;
  sv_lgvae_plan* p = new sv_lgvae_plan();
  p->d = *d;
  if (p->d.global_only) p->d.local_latent = p->d.global_latent;   // (ignored in this mode: keep the derived sizes well defined)
  p->params = build_params(d);
  p->nparams = p->params.back().off + (p->params.back().count + 3) / 4 * 4;
  p->bound = false;
  build_layers(p);
  for (int e = 0; e < 2 && !p->d.global_only; ++e)
    for (int l = 0; l < 4; ++l)
      if ((rc = svg_check(&p->enc[e][l].d))) { delete p; return rc; }
  for (int k = 0; k < p->ndec(); ++k)
    for (int l = 0; l < 5; ++l)
      if ((rc = svg_check(&p->dec[k][l].d))) { delete p; return rc; }
  build_prep_jobs(p);
  build_buffers(p);
  // the ranges the step zeroes with one memset each (phase_forward, phase_bwd_decoders, phase_bwd_encoders) hold exactly the buffers they name
  if (p->d.global_only ? !p->bufs.run(GZ, GZ) : !p->bufs.run(PRE, GZ_XH)) { delete p; return SV_E_STATE; }
  *out = p;
  return SV_OK;
}

extern "C" void sv_lgvae_plan_destroy(sv_lgvae_plan* p) {
  if (!p) return;
  p->prof.destroy();
  p->side.destroy();
  if (!p->graphs.empty()) (void)hipDeviceSynchronize();   // a replay may still be in flight
  for (auto& kv : p->graphs)
    if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
  delete p;
}

extern "C" int64_t sv_lgvae_workspace_bytes(const sv_lgvae_plan* p) { return p ? p->bufs.ws_bytes : -1; }

extern "C" int sv_lgvae_plan_bind(sv_lgvae_plan* p, void* workspace, int64_t bytes, void* stream) {
  if (!p) return SV_E_BADARG;
  SV_TRY(p->bufs.bind(workspace, bytes, (hipStream_t)stream, JOBS, p->jobs.data(), p->jobs.size() * sizeof(PrepJob)));
  p->bound = true;
  return SV_OK;
}

extern "C" int sv_lgvae_buffer(const sv_lgvae_plan* p, const char* name, int64_t* offset, int64_t* bytes) {
  return p ? p->bufs.lookup(name, offset, bytes) : SV_E_BADARG;
}

static int run_phases(sv_lgvae_plan* p, const sv_lgvae_step_args* s, hipStream_t st) {
  const int ph = s->phases;
  const bool capture = p->graph_on || p->dyn;
  p->side.begin_call(p->prof.serial(), capture, (ph & SV_PHASE_ALL) == SV_PHASE_ALL, p->ndec() * p->d.B);
  // early side work: the decoders' weight images and the gradient buffer's zero fill on side stream 0 beside the encoders' forward (see early_stream)
  const bool zero_here = (ph & SV_PHASE_LOSS) && s->grads;
  hipStream_t early = ((ph & SV_PHASE_PREP) && (ph & SV_PHASE_FWD_ENCODERS)) ? p->side.early_stream(st) : nullptr;
  if (early && zero_here) {
    if (hipMemsetAsync(s->grads, 0, (size_t)p->nparams * 4, early) != hipSuccess) return (int)hipGetLastError();
  }
  if (ph & SV_PHASE_PREP) SV_TRY(phase_prep(p, s, st, early));
  if (early) SV_TRY(p->side.early_done(early));
  static const bool no_fused_nll = SV_TUNE_FLAG("SV_NO_FUSED_NLL");    // A/B: dlogistic_kernel after the forward
  static const bool no_fused_nll_f32 = SV_TUNE_FLAG("SV_NO_FUSED_NLL_F32");    // (fp32 since round 6; A/B)
  const bool want_nll = !no_fused_nll && (ph & SV_PHASE_FWD_DECODERS) && (ph & SV_PHASE_LOSS) && s->grads && s->images6 &&
                        (p->d.dtype == SV_BF16 || !no_fused_nll_f32);
  if (!(ph & SV_PHASE_FORWARD)) p->nll_fused = false;
  if (ph & SV_PHASE_FORWARD) SV_TRY(phase_forward(p, s, ph & SV_PHASE_FWD_ENCODERS, ph & SV_PHASE_FWD_DECODERS, st, want_nll));
  if (ph & SV_PHASE_LOSS) {
    if (s->grads && !early) {
      Scope sc(p->prof, st, "zero_grads", 0, (double)p->nparams * 4);
      if (hipMemsetAsync(s->grads, 0, (size_t)p->nparams * 4, st) != hipSuccess) return (int)hipGetLastError();
    }
    SV_TRY(phase_loss(p, s, s->grads != nullptr, st));
  }
  SV_TRY(p->side.early_wait(st));                 // (a call without the decoders' forward: before any gradient is written, at the latest here)
  const bool buckets = (ph & SV_PHASE_BUCKET_EVENTS) && !capture;      // (not in captured steps: the events belong to eager launches)
  // a backward phase invalidates the events of every earlier step: sv_lgvae_bucket_wait must never succeed against events that belong to gradients
  // of a previous step (it returns SV_E_STATE instead, and the trainer falls back to ordering the collective behind the compute stream)
  if (ph & SV_PHASE_BACKWARD) p->side.clear_buckets();
  if (ph & SV_PHASE_BWD_DECODERS) {
    SV_TRY(phase_bwd_decoders(p, s, st));
    if (buckets) SV_TRY(p->side.record_bucket(0, st));
  }
  if (ph & (SV_PHASE_BWD_ENC_HEADS | SV_PHASE_BWD_ENC_CONVS))
    SV_TRY(phase_bwd_encoders(p, s, ph & SV_PHASE_BWD_ENC_HEADS, ph & SV_PHASE_BWD_ENC_CONVS, st, buckets));
  SV_TRY(p->side.join_side(st));
  if (ph & SV_PHASE_ADAM) {
    Scope sc(p->prof, st, "adam_step", 0, (double)p->nparams * 28);
    SV_TRY(svk_adam_step(s->params, s->grads, s->adam_m, s->adam_v, p->nparams, s->lr, s->beta1, s->beta2,
                         s->adam_eps, s->t, s->grad_scale, p->dyn, st));
  }
  return SV_OK;
}

// everything of a step that is baked into a captured graph: the phase mask, every buffer, every scalar that reaches a
// kernel as a launch argument.  seed / step / sample_offset / (lr, t) do not belong here: they travel through SvDynArgs.
static std::vector<uint64_t> graph_key(const sv_lgvae_plan* p, const sv_lgvae_step_args* s, hipStream_t st) {
  auto f = [](float x) { uint32_t u; memcpy(&u, &x, 4); return (uint64_t)u; };
  const bool adam = s->phases & SV_PHASE_ADAM;
  return {(uint64_t)(uint32_t)s->phases, (uint64_t)s->params, (uint64_t)s->grads, (uint64_t)s->adam_m, (uint64_t)s->adam_v,
          (uint64_t)s->images6, (uint64_t)s->eps_x, (uint64_t)s->eps_x_hat, (uint64_t)st,
          adam ? f(s->beta1) : 0, adam ? f(s->beta2) : 0, adam ? f(s->adam_eps) : 0, adam ? f(s->grad_scale) : 0,
          (uint64_t)s->accumulate_metrics, p->host_state_bits(), (uint64_t)p->buf(JOBS)};   // (JOBS: the workspace itself, its first buffer)
}

extern "C" int sv_lgvae_step(sv_lgvae_plan* p, const sv_lgvae_step_args* s, void* stream) {
  if (!p || !s) return SV_E_BADARG;
  if (!p->bound) return SV_E_STATE;
  hipStream_t st = (hipStream_t)stream;
  const int ph = s->phases;
  const bool train = ph & SV_PHASE_BACKWARD;
  if ((ph & (SV_PHASE_PREP | SV_PHASE_FORWARD | SV_PHASE_ADAM | SV_PHASE_BACKWARD)) && !s->params) return SV_E_BADARG;
  if ((ph & (SV_PHASE_FWD_ENCODERS | SV_PHASE_LOSS)) && !s->images6) return SV_E_BADARG;
  if (train && !s->grads) return SV_E_BADARG;
  if ((ph & SV_PHASE_ADAM) && (!s->grads || !s->adam_m || !s->adam_v || s->t <= 0)) return SV_E_BADARG;
  // no capture on the legacy default stream (HIP forbids it): callers that want replay run on a created stream
  if (!p->graph_on || p->prof.on || !st) return run_phases(p, s, st);

  // hipGraph replay: the first step with a given key runs eagerly (it also raises the kernels' dynamic-LDS caps, which
  // must not happen inside a capture), the second is captured, every later one is one graph launch.
  const std::vector<uint64_t> key = graph_key(p, s, st);
  if (p->graphs.size() >= 16 && !p->graphs.count(key)) return run_phases(p, s, st);   // callers that rotate buffers: stay eager
  sv_lgvae_plan::GraphEntry& e = p->graphs[key];
  if (!e.exec && e.seen++ == 0) return run_phases(p, s, st);
  const float alpha = (ph & SV_PHASE_ADAM) ? (float)svk_adam_alpha(s->lr, s->beta1, s->beta2, s->t) : 0.f;
  SV_TRY(svk_set_dyn((SvDynArgs*)p->buf(DYN), s->seed, s->step, s->sample_offset, alpha, st));
  if (!e.exec) {
    hipGraph_t g = nullptr;
    if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) != hipSuccess) return (int)hipGetLastError();
    p->dyn = (const SvDynArgs*)p->buf(DYN);
    const int rc = run_phases(p, s, st);
    p->dyn = nullptr;
    const hipError_t he = hipStreamEndCapture(st, &g);
    if (rc || he != hipSuccess || !g) {
      if (g) (void)hipGraphDestroy(g);
      return rc ? rc : (int)he;
    }
    const hipError_t hi = hipGraphInstantiate(&e.exec, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (hi != hipSuccess) { e.exec = nullptr; return (int)hi; }
    e.exit_state = p->host_state();              // what the captured phases left behind (the entry state is part of the key)
  } else {
    p->set_host_state(e.exit_state);             // the host-side state the replayed phases would have left behind
  }
  if (hipGraphLaunch(e.exec, st) != hipSuccess) return (int)hipGetLastError();
  return SV_OK;
}

extern "C" int sv_lgvae_graph_enable(sv_lgvae_plan* p, int32_t enable) {
  if (!p) return SV_E_BADARG;
  if (enable && p->d.global_only) return SV_E_UNSUPPORTED;   // GMVae steps interleave the caller's encoder between the plan's phases: no capture path
  p->graph_on = enable != 0;
  if (!enable) {
    for (auto& kv : p->graphs)
      if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
    p->graphs.clear();
  }
  return SV_OK;
}

extern "C" int sv_lgvae_bucket_wait(sv_lgvae_plan* p, int32_t bucket, void* stream) {
  if (!p || bucket < 0 || bucket > 3) return SV_E_BADARG;
  return p->side.bucket_wait(bucket, (hipStream_t)stream);
}

// per-plan test hooks (SideStreams::debug)
extern "C" int sv_lgvae_plan_debug(sv_lgvae_plan* p, const char* key, int64_t value) {
  if (!p || !key) return SV_E_BADARG;
  return p->side.debug(key, value);
}

// test hook: the dz state machine of the latent block (plan_latent.h) as plain integers; no device call
extern "C" int sv_lgvae_dz_transition(int32_t state, int32_t event, int32_t slab_path, int32_t* next, int32_t* zero_range) {
  if (state < 0 || state > 3 || event < 0 || event > 3 || !next || !zero_range) return SV_E_BADARG;
  const DzStep t = dz_transition((DzState)state, (DzEvent)event, slab_path != 0);
  *next = (int32_t)t.next;
  *zero_range = (int32_t)t.zero;
  return SV_OK;
}

extern "C" int sv_lgvae_graph_count(const sv_lgvae_plan* p) {
  if (!p) return SV_E_BADARG;
  int n = 0;
  for (auto& kv : p->graphs) n += kv.second.exec != nullptr;
  return n;
}

extern "C" int sv_lgvae_profile_enable(sv_lgvae_plan* p, int32_t enable) {
  if (!p) return SV_E_BADARG;
  p->prof.enable(enable != 0);
  return SV_OK;
}

extern "C" int sv_lgvae_profile_filter(sv_lgvae_plan* p, const char* name) {
  if (!p) return SV_E_BADARG;
  p->prof.filter = name ? name : "";
  return SV_OK;
}

extern "C" int sv_lgvae_profile_read(sv_lgvae_plan* p, int32_t max_entries, char names[][64], double* total_ms,
                                     int32_t* launches, double* flops_per_launch, double* bytes_per_launch) {
  if (!p) return SV_E_BADARG;
  return p->prof.read(max_entries, names, total_ms, launches, flops_per_launch, bytes_per_launch);
}

extern "C" int sv_lgvae_profile_read_issued(sv_lgvae_plan* p, int32_t max_entries, double* issued_flops_per_launch) {
  if (!p || !issued_flops_per_launch) return SV_E_BADARG;
  return p->prof.read_issued(max_entries, issued_flops_per_launch);
}

extern "C" const char* sv_version(void) { return "splitvae-hip 0.1 (gfx950)"; }

extern "C" int sv_set_deterministic(int32_t mode) {
  if (mode < -1 || mode > 1) return SV_E_BADARG;
  sv_deterministic_override().store(mode, std::memory_order_relaxed);
  return SV_OK;
}

extern "C" int sv_get_deterministic(void) { return sv_deterministic() ? 1 : 0; }
