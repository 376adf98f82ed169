// The launch plan of the spliced GEMM (gemm_plan.h): argument checks, mode rules, kernel choice, partition, K-walk groups.
#include "gemm_plan.h"

#include <stdio.h>

#include <algorithm>

namespace xv {

GemmPolicy MakeGemmPolicy(int cus, int variant, int sk_mf, int sk_lanes, int stagger_pct) {
  return {cus, (variant != 0 && variant != 1 && variant != 2 && variant != 4) ? 0 : variant, (sk_mf != 4 && sk_mf != 8) ? 8 : sk_mf,
          (sk_lanes != 1 && sk_lanes != 2 && sk_lanes != 4) ? 4 : sk_lanes, stagger_pct};
}

// Groups consecutive K segments that read the same source at uniformly spaced time offsets (see the v2 kernel); the
// grouping rule itself is PlanWalkGroups (kernels.h), shared with the host code that packs weights in walk order.
// second_walk (kPrecFp16Mx2): behind the first ones the groups of the second K walk - the same sources, time offsets and order,
// steps of 128 columns over the 4-bit residual planes (as 16-bit elements: a quarter of the row pitch and of the steps).
static void BuildWalkGroups(GemmArgs* g, bool second_walk) {
  long key[kMaxSeg];
  int shift[kMaxSeg], ksteps[kMaxSeg];
  for (int j = 0; j < g->nseg; ++j) {
    key[j] = j;
    for (int k = 0; k < j; ++k)
      if (g->seg[k].hi == g->seg[j].hi && g->seg[k].lo == g->seg[j].lo && g->seg[k].ld == g->seg[j].ld) {
        key[j] = key[k];
        break;
      }
    shift[j] = g->seg[j].row_shift;
    ksteps[j] = g->seg[j].ksteps;
  }
  WalkGroup wg[kMaxSeg];
  g->ngrp = PlanWalkGroups(g->nseg, key, shift, ksteps, wg);
  g->ngrp_lo = second_walk ? g->ngrp : 0;
  g->lo_ksteps = 0;
  for (int i = 0; i < g->ngrp; ++i) {
    const Seg& s0 = g->seg[wg[i].first_seg];
    Grp& G = g->grp[i];
    G = Grp();
    G.hi = s0.hi;
    G.lo = s0.lo;
    G.ld = s0.ld;
    G.ksteps = wg[i].ksteps;
    G.nshift = wg[i].nshift;
    G.shift0 = wg[i].shift0;
    G.dstep = wg[i].dstep;
    G.wcol0 = wg[i].wcol0;
    G.wstride = wg[i].wstride;
    G.gmax = s0.gmax;
    if (!second_walk) continue;
    Grp& L = g->grp[g->ngrp + i];
    L = G;
    L.hi = (const uint16_t*)s0.lo4;
    L.lo = nullptr;
    L.ld = s0.ld / 4;
    L.ksteps = G.ksteps / 4;
    L.gmax = nullptr;
    L.lo4s = s0.lo4s;
    L.ld4s = Lo4ScalePitch(s0.ld);
    g->lo_ksteps += L.ksteps * L.nshift;
  }
}

// The applicability rules on arguments whose first-walk groups are built
static bool MxOk(const GemmArgs& b) {
  if (!b.w4 || !b.w4_scale || b.ldw4 <= 0 || (b.m_tiles & 1) || (b.total_ksteps & 3)) return false;
  for (int i = 0; i < b.ngrp; ++i)
    if (!b.grp[i].gmax || (b.grp[i].ksteps * b.grp[i].nshift) % 4) return false;
  return true;
}

static bool Mx2Ok(const GemmArgs& b) {
  if (!MxOk(b) || !b.w4b || !b.w4b_scale || b.ldw4b <= 0) return false;
  for (int i = 0; i < b.ngrp; ++i)   // whole 128-column steps
    if (b.grp[i].ksteps % 4 || b.grp[i].ld % 128) return false;
  for (int j = 0; j < b.nseg; ++j)
    if (!b.seg[j].lo4 || !b.seg[j].lo4s) return false;
  return true;
}

// tdnn_gemm_kernel_p8 can run this launch: whole 256 x 256 tiles, every K group a whole number of 64-column tiles (of
// 128-column blocks for kPrecFp16Mx), an even number of K tiles, and for kPrecFp16Mx the residual plane in ITS walk order
// (GemmArgs::p8 is the caller's statement that w4 / w4_scale are in that order).  *ktiles: the K tiles of an output tile.
static bool P8Ok(const GemmArgs& b, int precision, int* ktiles) {
  if (precision == kPrecFp16MxE) precision = kPrecFp16Mx;   // the same product; its planes epilogue also writes the residual plane
  if (precision != kPrecFp16 && precision != kPrecFp16Mx && precision != kPrecFp16Mx2) return false;
  if ((b.m_tiles & 1) || (b.n_tiles & 1) || b.ksplit > 1) return false;
  const bool mx = precision != kPrecFp16, mx2 = precision == kPrecFp16Mx2;
  int t = 0;
  for (int i = 0; i < b.ngrp; ++i) {
    // whole K tiles: 64 columns; whole blocks of the residual product: 128; whole tiles of the second walk: 256
    if (b.grp[i].ksteps % (mx2 ? 8 : mx ? 4 : 2) || b.grp[i].ld % (mx2 ? 256 : 64)) return false;
    if (mx && !b.grp[i].gmax) return false;
    t += (b.grp[i].ksteps >> 1) * b.grp[i].nshift;
  }
  if (t < 2 || (t & 1)) return false;
  if (mx && (!b.w4 || !b.w4_scale || b.ldw4 <= 0)) return false;
  if (mx2) {
    if (!b.w4b || !b.w4b_scale || b.ldw4b <= 0) return false;
    for (int j = 0; j < b.nseg; ++j)
      if (!b.seg[j].lo4 || !b.seg[j].lo4s) return false;
  }
  *ktiles = t;
  return true;
}

static bool WithGroups(const GemmArgs& a, GemmArgs* b) {
  if (a.nseg < 1 || a.nseg > kMaxSeg) return false;
  *b = a;
  BuildWalkGroups(b, false);
  return true;
}
bool gemm_mx_applicable(const GemmArgs& a) { GemmArgs b; return WithGroups(a, &b) && MxOk(b); }
bool gemm_mx2_applicable(const GemmArgs& a) { GemmArgs b; return WithGroups(a, &b) && Mx2Ok(b); }
bool gemm_p8_applicable(const GemmArgs& a, int precision) { GemmArgs b; int t; return WithGroups(a, &b) && P8Ok(b, precision, &t); }

// True when the stream-K variant with mf fragments per wave can run this launch.
static bool SkApplicable(const GemmArgs& a, int prec, int mf, int cus) {
  if (GemmSkLds(prec, mf) > kGemmMaxLds) return false;
  const int rows = a.m_tiles * kBM;
  if (rows % (64 * mf)) return false;
  const int grid = cus / 8 * 8;
  if (grid < 8) return false;
  // every workgroup gets at least one tile's worth of K steps (XCD blocks are whole row tiles) ...
  if ((long)(rows / (64 * mf) / 8) * a.n_tiles >= grid / 8) return true;
  // ... or, on fewer workgroups (see PlanPersistent), launches between the two regimes: at least four row tiles per XCD block, and
  // more 256-row tiles than the per-tile kernel finishes in one round (48 and 64 chunks of 400 frames: 300 / 400 tiles of
  // tdnn2 on 256 CUs = two rounds, 82 us for both, where one round is 42)
  return mf == 8 && rows / (64 * mf) / 8 >= 4 && (long)(a.m_tiles / 2) * a.n_tiles > cus;
}

// The persistent kernels (stream-K, p8): `lanes` column lanes over the launch's ntiles column tiles; workgroup groups per XCD block
// and lane: as many as the CUs allow, but not more than the block has tiles per lane (every group's share must hold at least one
// whole tile).  Needs GemmArgs::sk_mtiles.
static void PlanPersistent(GemmPlan* p, int cus, int ntiles, int lanes, int lds, size_t slot_bytes) {
  const int tiles_min = std::max(1, (p->args.sk_mtiles / 8) * (ntiles / lanes));
  p->args.sk_lanes = lanes;
  p->grid_x = 8 * lanes * std::min(cus / 8 / lanes, tiles_min);
  p->block = 512;
  p->lds = lds;
  p->sk_ws_bytes = (size_t)p->grid_x * slot_bytes;
}

GemmPlan PlanGemm(const GemmArgs& a, int prec, int epi, const GemmPolicy& pol) {
  GemmPlan p = {};
  p.precision = prec;
  p.epilogue = epi;
  p.grid_y = 1;
  p.args = a;
  GemmArgs& b = p.args;
  if (a.nseg < 1 || a.nseg > kMaxSeg || a.m_tiles < 1 || a.n_tiles < 1) return p;
  // what a mode can write
  switch (prec) {
    case kPrecFp16x3E: case kPrecFp16MxE:   // planes out only (the layers, and the 1.25-pass product, in front of a kPrecFp16Mx2 consumer)
      if (a.ksplit > 1 || epi != kEpiAct || !a.out_lo4 || !a.out_lo4s) return p;
      break;
    case kPrecFp16Mx: case kPrecFp16Mx2:   // frame-level layers only: planes out or pooled statistics
      if (a.ksplit > 1 || (epi != kEpiAct && epi != kEpiStats)) return p;
      break;
    case kPrecBf16x3: case kPrecBf16: case kPrecFp16: case kPrecFp16x3: case kPrecFp16x2:
      if (epi != kEpiAct && epi != kEpiF32 && epi != kEpiStats) return p;
      break;
    default: return p;
  }
  if (a.ksplit > 1 && a.splitk_ws) {
    if (epi == kEpiStats) return p;
    p.kernel = kGemmSplitK;
    p.grid_x = a.m_tiles * a.n_tiles;
    p.grid_y = a.ksplit;
    p.block = 256;
    p.lds = GemmTileLds(prec, kSplitKStages);
    p.ok = true;
    return p;
  }
  BuildWalkGroups(&b, PrecMx2(prec));
  const int cus8 = pol.cus / 8 * 8;
  if (a.p8) {   // the caller packed / chose this layer for the 64-column K walk: no other kernel accumulates in that order
    const bool built = ((prec == kPrecFp16 || prec == kPrecFp16Mx || prec == kPrecFp16Mx2) && (epi == kEpiAct || epi == kEpiStats)) ||
                       (prec == kPrecFp16MxE && epi == kEpiAct);
    if (!built || !P8Ok(b, prec, &b.p8_ktiles) || cus8 < 8) return p;
    b.p8_ktiles_lo = 0;   // second walk: the 4-bit planes, steps of 128 columns (a tile = two of them)
    for (int i = 0; i < b.ngrp_lo; ++i) b.p8_ktiles_lo += (b.grp[b.ngrp + i].ksteps >> 1) * b.grp[b.ngrp + i].nshift;
    b.p8 = 1;
    // GemmArgs::p8_whole as the caller's policy (Engine: XVEC_DEBUG=p8_whole): 0 = K tiles dealt out evenly over the workgroups (stream-K
    // exchange; the default), 1 = whole tiles for every launch, 2 = whole tiles for layers of at most 8 K tiles per output tile
    b.p8_whole = (a.p8_whole == 1 || (a.p8_whole == 2 && b.p8_ktiles + b.p8_ktiles_lo <= 8)) ? 1 : 0;
    b.sk_mtiles = a.m_tiles >> 1;
    const int nt = a.n_tiles >> 1;
    // column lanes: the largest of 4, 2, 1 that divides the column tiles and the workgroups of an XCD block
    int l = 4;
    while (l > 1 && (nt % l || (cus8 / 8) % l)) l >>= 1;
    // Column tiles in threes (1536 = 6, 768 = 3 tiles of 256: the statistics layer, the 650-wide layers of the c-vector network):
    // with two lanes - or one - every workgroup walks its row tile's frames once per column tile, 16 to 32 row tiles are in flight
    // per XCD (4 - 8 MB of frames against 4 MB of L2), and every pass after the first misses: 578 MB per tdnn5 launch for a 105 MB
    // plane (profiles/r05w_pmc_hbm.md).  As many lanes as column tiles instead: the lanes of a group walk the SAME row tile at the
    // same time, the first brings a line into the XCD's L2 and the others find it there.  The workgroups of an XCD block are
    // then a multiple of 3 (30 of 32 CUs); the partition is bit-identical whatever the cut.
    // (same box, A/B: tdnn5 of the x-vector 572 -> 245 MB per launch at the same 0.205 ms; the 768-wide layers of the c-vector
    // network 1141 -> 330 MB and 721 -> 285 MB, their launches +2.5 % on their own and the two-lane step -3.5 % - profiles/r06_lanes.md)
    if (nt % 3 == 0 && nt <= 6 && cus8 / 8 >= nt) l = nt;
    p.kernel = kGemmP8;
    PlanPersistent(&p, cus8, nt, l, GemmP8Lds(), (size_t)256 * 256 * sizeof(float));
    p.ok = true;
    return p;
  }
  // default policy (same box, 256 x 400 workload): two-pass mode - stream-K for every layer; three-pass and single-pass
  // modes - stream-K only for the long-K layers (tdnn2 / tdnn3, 48 K steps: -5 % / -9 %), the short-K ones are faster
  // on the per-tile kernel there (tdnn5 single-pass: 0.190 vs 0.229 ms)
  const bool sk_default = prec == kPrecFp16x2 || prec == kPrecFp16Mx || a.total_ksteps >= 32;
  int mf = 0;
  if (PrecMx(prec)) {
    // 512-row stream-K tiles or the 256-row per-tile kernel (bit-identical); nothing else implements the mode
    if (PrecMx2(prec) ? !Mx2Ok(b) : !MxOk(b)) return p;
    if (pol.variant != 2 && pol.variant != 1 && pol.sk_max_mf == 8 && SkApplicable(a, prec, 8, pol.cus)) mf = 8;
    p.kernel = mf ? kGemmSk : kGemmV2;
  } else {
    if (pol.variant == 4 || (pol.variant == 0 && sk_default)) {
      if (pol.sk_max_mf == 8 && SkApplicable(a, prec, 8, pol.cus)) mf = 8;
      else if ((pol.variant == 4 || PrecXPlanes(prec) == 2) && SkApplicable(a, prec, 4, pol.cus)) mf = 4;
    }
    p.kernel = mf ? kGemmSk : (pol.variant != 1 && (a.m_tiles & 1) == 0) ? kGemmV2 : kGemmTile;
  }
  p.ok = true;
  if (p.kernel == kGemmSk) {
    p.mf = mf;
    b.sk_mtiles = a.m_tiles * kBM / (64 * mf);
    // column lanes: the largest of 4, 2, 1 that divides the column tiles and the workgroups of an XCD block
    int l = pol.sk_max_lanes;
    while (l > 1 && (a.n_tiles % l || (cus8 / 8) % l)) l >>= 1;
    PlanPersistent(&p, cus8, a.n_tiles, l, GemmSkLds(prec, mf), (size_t)64 * mf * kBN * sizeof(float));
  } else if (p.kernel == kGemmV2) {
    const int mt8 = ((a.m_tiles >> 1) + 7) / 8 * 8;
    p.grid_x = mt8 * a.n_tiles;
    p.block = 512;
    p.lds = GemmV2Lds(prec);
    // stagger window = gemm_stagger (XVEC_DEBUG) percent of the modelled tile time (K steps x ~2200 cycles in split mode,
    // ~1000 single pass, + ~14000 fixed)
    b.stagger_wgs = pol.cus;
    b.stagger_units = (p.grid_x > 2 * pol.cus) ? (int)(((long)b.total_ksteps * (400 + 600 * PrecPasses(prec)) + 14000) * pol.stagger_pct / 100 / 2048) : 0;
  } else {
    p.grid_x = (a.m_tiles + 7) / 8 * 8 * a.n_tiles;
    p.block = 256;
    p.lds = GemmTileLds(prec, 2);
  }
  return p;
}

void GemmKernelName(const GemmPlan& p, char* buf, size_t cap) {
  static const char* const prec_name[] = {"bf16x3", "bf16", "fp16", "fp16x3", "fp16x2", "auto", "fp16mx", "fp16mx2", "fp16x3e", "fp16mxe"};
  static const char* const epi_name[] = {"act", "f32", "stats", "splitk"};
  static const char* const variant[] = {"", "_v2", "_sk", "_p8", ""};
  const char* pn = (p.precision >= 0 && p.precision <= 9) ? prec_name[p.precision] : "?";
  const char* en = epi_name[p.kernel == kGemmSplitK ? (int)kEpiSplitK : (p.epilogue & 3)];
  if (p.mf) snprintf(buf, cap, "tdnn_gemm_kernel%s<%s,%s,%d>", variant[p.kernel], pn, en, p.mf);
  else snprintf(buf, cap, "tdnn_gemm_kernel%s<%s,%s>", variant[p.kernel], pn, en);
}

}  // namespace xv
