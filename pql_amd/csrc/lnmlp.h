// What the whole-stack launches of the LayerNorm twin critic share on the host: the forward of fwd_ln.hip and the input-gradient pass
// of bwd_ln.hip read the same arena, the same stash slab and the same LDS image, so the layout of all three is stated once, here.
// (The block geometry and what the residual critic's launches share too: lnstack.h.)
#pragma once
#include "lnstack.h"

// the arena law of the normalised twin critics (include/pqlk.h): per net and layer [W | b], then [gamma | beta] behind a hidden one
struct LmLayout {
  int n_layers, n_nets;
  int dims[PQLK_MAX_LAYERS + 1];
  int64_t lin_off[PQLK_MAX_LAYERS], gamma_off[PQLK_MAX_LAYERS], beta_off[PQLK_MAX_LAYERS], net_stride;
};

static int lm_image_cols(const LmLayout* d) {
  int w = (int)pqlk_ld(d->dims[0]);
  for (int l = 1; l < d->n_layers; ++l) w = w > d->dims[l] ? w : d->dims[l];
  return w;
}
static size_t lm_lds_bytes(const LmLayout* d, int r) { return ls_lds_bytes(lm_image_cols(d), r); }

// the layout of an eligible descriptor -> *out; false: not eligible
static bool lm_layout(const PqlMlpDesc* m, LmLayout* out) {
  if (desc_ok(m) != PQLK_OK || m->n_layers < 2 || m->dims[m->n_layers] != 1) return false;
  for (int l = 1; l < m->n_layers; ++l)
    if (m->dims[l] % 32 != 0 || m->dims[l] > 1024) return false;
  LmLayout d = {};
  d.n_layers = m->n_layers; d.n_nets = m->n_nets;
  int64_t o = 0;
  for (int l = 0; l < d.n_layers; ++l) {
    d.dims[l] = m->dims[l]; d.dims[l + 1] = m->dims[l + 1];
    d.lin_off[l] = o;
    o += (int64_t)m->dims[l + 1] * pqlk_ld(m->dims[l]) + pqlk_ld(m->dims[l + 1]);
    if (l < d.n_layers - 1) {
      d.gamma_off[l] = o; d.beta_off[l] = o + pqlk_ld(m->dims[l + 1]);
      o += 2 * pqlk_ld(m->dims[l + 1]);
    }
  }
  d.net_stride = o;
  if (lm_lds_bytes(&d, 1) > (size_t)LS_LDS_MAX) return false;   // (bounds the input width: ld(dims[0]) <= 1248)
  *out = d;
  return true;
}

// a net's stash: z, y of every hidden layer, (m, dims[l + 1]) each, then mean, rstd of every hidden layer, m floats rounded up to 4
static int64_t lm_stash_net_floats(const LmLayout* d, int64_t m) {
  int64_t o = 0;
  for (int l = 1; l < d->n_layers; ++l) o += 2 * m * d->dims[l] + 2 * ls_round4(m);
  return o;
}

// where `which` of hidden layer `layer` of net 0 starts in a stash of m rows, and its row stride
static void lm_stash_at(const LmLayout* d, int64_t m, int layer, int which, int64_t* off, int64_t* ld) {
  int64_t o = 0;
  if (which <= PQLK_LNMLP_Y) {
    for (int l = 0; l < layer; ++l) o += 2 * m * d->dims[l + 1];
    *off = o + (which == PQLK_LNMLP_Y ? m * d->dims[layer + 1] : 0);
    *ld = d->dims[layer + 1];
  } else {
    for (int l = 1; l < d->n_layers; ++l) o += 2 * m * d->dims[l];
    *off = o + (2 * layer + (which == PQLK_LNMLP_RSTD ? 1 : 0)) * ls_round4(m);
    *ld = 1;
  }
}
