// conv_plan.h -- what the split-fp16 convolution hosts launch for a shape: kernel form, tile height, slab grouping.  HOST code, pure
// functions of (shape, knobs, CU count): no HIP call, and read_conv_knobs() is the only place these hosts read the environment.
// The launch functions (conv_f16_wx4.hip, conv_f16.hip, conv_f16_s2.hip, conv_f16_pw.hip) execute the plan; virnet_conv_plan_query
// returns it without launching (tests/test_launch_plan.py holds every rule below to a recorded table).
#pragma once
#include <stdlib.h>
#include "../../include/virnet_hip.h"

namespace virnet {

typedef virnet_conv_launch ConvLaunch;      // { form, rows, ng, nrep, variant, slab_base, groups, persistent }: groups * ng * nrep slabs from slab_base on

struct ConvPlan {
  int n = 0;
  ConvLaunch l[4];                           // (the stride-2 and the transposed host can take four launches, the others at most three)
  // a launch of `groups` channel blocks; none for an empty group, -1 when the plan is full
  int add(int form, int rows, int ng, int nrep, int variant, int slab_base, int groups, int persistent = 0) {
    if (groups <= 0) return 0;
    if (n == 4) return -1;
    l[n++] = ConvLaunch{form, rows, ng, nrep, variant, slab_base, groups, persistent};
    return 0;
  }
};

struct ConvShape { int n, h, w, nb; };       // images, OUTPUT rows / columns the tiles cover, 32-channel slabs

// tiles of `rows` x 32 pixels over n images
inline long tiles(int n, int h, int w, int rows) { return (long)n * ((h + rows - 1) / rows) * ((w + 31) / 32); }

// Slabs per workgroup: 3 where the count allows, the remainder in 2s (160 channels = 3 + 2, 224 = 3 + 2 + 2: two launches, each
// staging the pixel tile once per workgroup, instead of 5 / 7 single-slab workgroups per tile); a lone odd slab runs by itself.
struct SlabGroups { int n3, n2, n1; };
inline SlabGroups slab_groups(int nb) {
  int n3 = nb / 3, rem = nb - 3 * n3;
  if (rem == 1 && n3 >= 1) { n3 -= 1; rem = 4; }
  const int n2 = rem / 2;
  return {n3, n2, rem - 2 * n2};
}
// One level up (stride-2 and transposed conv): 6 (8 waves) where the count allows, then 3 / 2 / 1 with 4 waves (288 channels = 6 + 3,
// 160 = 3 + 2, 224 = 6 + ... 3 + 2 + 2); max_group < 6 / < 3 takes the larger groups away.
struct SlabGroups6 { int n6, n3, n2, n1; };
inline SlabGroups6 slab_groups6(int nb, int max_group) {
  int n6 = nb / 6, rem = nb - 6 * n6;
  if (max_group < 6) { n6 = 0; rem = nb; }
  if (rem == 1 && n6 >= 1) { n6 -= 1; rem = 7; }
  int n3 = rem / 3, rem2 = rem - 3 * n3;
  if (max_group < 3) { n3 = 0; rem2 = rem; }
  if (rem2 == 1 && n3 >= 1) { n3 -= 1; rem2 = 4; }
  const int n2 = rem2 / 2;
  return {n6, n3, n2, rem2 - 2 * n2};
}
inline int add_groups6(ConvPlan& p, int form, int rows, int variant, const SlabGroups6& g) {
  int base = 0, rc = 0;
  const int ng[4] = {2, 1, 1, 1}, nrep[4] = {3, 3, 2, 1}, groups[4] = {g.n6, g.n3, g.n2, g.n1};
  for (int i = 0; i < 4 && rc == 0; ++i) {
    rc = p.add(form, rows, ng[i], nrep[i], variant, base, groups[i]);
    base += groups[i] * ng[i] * nrep[i];
  }
  return rc;
}

// epilogue class (4: two stored tensors and / or SFT on the output; else residual | 2 * mask) and pre-activation class (2: SFT, 1: LeakyReLU)
inline int epi_of(const virnet_conv_desc* d) { return (d->mul || (d->y_raw && d->y_act)) ? 4 : (d->res ? 1 : 0) | (d->mask ? 2 : 0); }
inline int pre_of(const virnet_conv_desc* d) { return d->in_mul ? 2 : (d->in_act != 0); }

// The library-side knobs of these hosts (tools/knobs.md).  Read per call -- tests and A/B runs flip them inside one process -- except the
// two `static` ones.  A host reads its own family's knobs only: the single-image path is host-bound.
struct ConvKnobs {
  bool wx4_alt;                 // VIRNET_WX4_ALT=1 (once per process)
  bool wx4_nrep_set;            // VIRNET_WX4_NREP is present,
  int wx4_nrep;                 // ... and its value (0: the default grouping)
  int wx4_rows_pin;             // VIRNET_WX4_ROWS, else 16 under VIRNET_DETERMINISTIC=1 / VIRNET_WX4_MIN_WGS=0, else 0
  bool wx4_wide_off;            // VIRNET_WX4_WIDE=0 (consulted for five slabs only)
  bool wx4_persist;             // VIRNET_WX4_PERSIST=1
  int wx4_persist_min;          // VIRNET_WX4_PERSIST_MIN (default 2)
  int f16_mrep;                 // VIRNET_F16_MREP (0: by launch size)
  bool f16_split_set;           // VIRNET_F16_SPLIT_WGS is present,
  long f16_split_wgs;           // ... and its value
  bool s2_wide_off;             // VIRNET_S2_WIDE=0 (once per process)
  long s2_split_tiles;          // VIRNET_S2_SPLIT_TILES (default 64)
  bool convt_ks3;               // VIRNET_CONVT_KS=3
  int convt_slabs;              // VIRNET_CONVT_SLABS (default 6)
};
enum { KNOBS_WX4, KNOBS_F16, KNOBS_S2, KNOBS_CONVT };
inline ConvKnobs read_conv_knobs(int host, int nb = 0) {
  ConvKnobs k{};
  if (host == KNOBS_WX4) {
    static const bool alt = getenv("VIRNET_WX4_ALT") && getenv("VIRNET_WX4_ALT")[0] == '1';
    k.wx4_alt = alt;
    const char* const nrep_env = getenv("VIRNET_WX4_NREP");
    k.wx4_nrep_set = nrep_env != nullptr;
    k.wx4_nrep = nrep_env ? atoi(nrep_env) : 0;
    // VIRNET_DETERMINISTIC=1 (or the older VIRNET_WX4_MIN_WGS=0): results must not depend on the launch size -> one tile form for all.
    const char* const rows_env = getenv("VIRNET_WX4_ROWS");
    const char* const det_env = getenv("VIRNET_DETERMINISTIC");
    const char* const wgs_env = getenv("VIRNET_WX4_MIN_WGS");
    k.wx4_rows_pin = rows_env ? atoi(rows_env) : ((det_env && det_env[0] == '1') || (wgs_env && wgs_env[0] == '0' && wgs_env[1] == 0)) ? 16 : 0;
    k.wx4_wide_off = nb == 5 && getenv("VIRNET_WX4_WIDE") && getenv("VIRNET_WX4_WIDE")[0] == '0';
    const char* const pe = getenv("VIRNET_WX4_PERSIST");
    k.wx4_persist = pe && pe[0] == '1';
    const char* const pm = k.wx4_persist ? getenv("VIRNET_WX4_PERSIST_MIN") : nullptr;
    k.wx4_persist_min = pm ? atoi(pm) : 2;
  } else if (host == KNOBS_F16) {
    const char* const env_m = getenv("VIRNET_F16_MREP");      // tuning / tests
    k.f16_mrep = env_m ? atoi(env_m) : 0;
    const char* const env_s = getenv("VIRNET_F16_SPLIT_WGS");
    k.f16_split_set = env_s != nullptr;
    k.f16_split_wgs = env_s ? atol(env_s) : 0;
  } else if (host == KNOBS_S2) {
    static const bool wide_off = getenv("VIRNET_S2_WIDE") && getenv("VIRNET_S2_WIDE")[0] == '0';      // (A/B knob)
    k.s2_wide_off = wide_off;
    const char* const env_t = getenv("VIRNET_S2_SPLIT_TILES");
    k.s2_split_tiles = env_t ? atol(env_t) : 64;
  } else {
    const char* const ks_env = getenv("VIRNET_CONVT_KS");
    k.convt_ks3 = ks_env && atoi(ks_env) == 3;
    const char* const f = getenv("VIRNET_CONVT_SLABS");      // tuning aid: largest slab group per workgroup (6 default, 3, 2)
    k.convt_slabs = f ? atoi(f) : 6;
  }
  return k;
}

// ---- virnet_conv_wx4 (conv_f16_wx4.hip / _wx4h.hip / _wx4p.hip) ---------------------------------------------------------------
// emit_rows: 0, or the tile height the caller of virnet_conv_wx4_emit asked for (8 / 16); wx4p_ok: the persistent form serves the
// shape's three-slab launch (wx4p_serves)
inline int plan_wx4(const ConvShape& s, int pre, int emit_rows, const ConvKnobs& kn, int n_cu, bool wx4p_ok, ConvPlan& p) {
  const int nb = s.nb, rows_pin = kn.wx4_rows_pin;
  SlabGroups g = slab_groups(nb);
  // Launches that leave CUs empty (the deep levels of a single image: 128x128x192 is 64 8-row tiles x 2 channel blocks): fewer slabs per
  // workgroup -- the smallest count that still fits ONE round of one workgroup per CU in ONE launch (measured, profiles/r04_probes.md 7:
  // q1 3/2/1 slabs 0.052 / 0.046 / 0.051 ms, q2 0.062 / 0.084 (two launches) / 0.047, r1 0.049 / 0.041 / 0.037).  No result bit depends on
  // the grouping.  VIRNET_WX4_NREP=1|2|3 pins it (3 = the default grouping).
  int want = kn.wx4_nrep;
  if (want == 0) {
    const long tiles8 = tiles(s.n, s.h, s.w, 8);
    if (tiles8 * (g.n3 + g.n2 + g.n1) < n_cu) {
      for (int c = 1; c <= 2 && want == 0; ++c)
        if (nb % c == 0 && tiles8 * (nb / c) <= n_cu) want = c;
    }
  }
  if (want == 1) g = {0, 0, nb};
  else if (want == 2) g = {0, nb / 2, nb - 2 * (nb / 2)};
  // Tile form per launch: 16-row tiles / 8 waves / one workgroup per CU (conv_f16_wx4.hip) or 8-row tiles / 4 waves / two per CU
  // (conv_f16_wx4h.hip).  Measured (profiles/r04_probes.md): on launches that fill the chip many times over both forms run the socket
  // at its 1400 W power cap and the 16-row form is 3-6 % ahead (fewer barriers and weight pieces per MFMA) -- except with two-slab
  // workgroups (64 channels), where the 8-row form is 4 % ahead; on launches of a few hundred workgroups the 8-row form wins whenever
  // its finer grain saves a round: a lone 8-row workgroup takes ~0.55 of a 16-row one, a co-resident pair ~1.04.
  // VIRNET_WX4_ROWS=8|16 pins the form (A/B runs, tests).
  auto half_tiles_for = [&](int nrep, int groups) -> bool {
    if (rows_pin == 8) return true;
    if (rows_pin == 16) return false;
    const long w16 = tiles(s.n, s.h, s.w, 16) * groups;
    const long w8 = tiles(s.n, s.h, s.w, 8) * groups;
    if (pre == 2 && nrep == 3) return w8 <= n_cu;              // (the 8-row form's 80 KB have no room for the SFT table next to three slabs: one
                                                               //  workgroup per CU -- which is all a launch of at most n_cu workgroups asks for: SISR, one image)
    if (w16 >= 8L * n_cu) return nrep <= 2;                     // chip filled many times over
    const double t16 = (double)((w16 + n_cu - 1) / n_cu);
    const long full = w8 / (2L * n_cu), tail = w8 - full * 2L * n_cu;
    const double t8 = 1.04 * (double)full + (tail == 0 ? 0.0 : tail <= n_cu ? 0.55 : 1.04);
    return t8 < t16;
  };
  auto one = [&](int nrep, int slab_base, int groups) -> int {
    if (emit_rows == 8) return p.add(VIRNET_LAUNCH_WX4H, 8, 1, nrep, 0, slab_base, groups);
    if (emit_rows) return p.add(VIRNET_LAUNCH_WX4, 16, 1, nrep, 0, slab_base, groups);      // emission: the tile form the caller asked for, whatever the launch size
    if (nrep == 5 || half_tiles_for(nrep, groups)) return p.add(VIRNET_LAUNCH_WX4H, 8, 1, nrep, 0, slab_base, groups);
    // 16-row tiles, persistent form (conv_f16_wx4p.hip, round 6: one workgroup per CU walks its XCD's items, the next item's first chunk is
    // staged by the last chunk's stages, the epilogue's exchange leaves V and weight buffer 0 alone).  BUILT, bit-identical, and measured:
    // no prologue (10.9 k of a tile's 71.4 k cycles), and 2-3 % MORE time per launch / 1.7 % fewer images per second end to end: with every CU
    // streaming all the time each stage takes 6 % longer (profiles/r06_probes.md 2).  Therefore opt-in: VIRNET_WX4_PERSIST=1, for launches of
    // at least VIRNET_WX4_PERSIST_MIN (default 2) items per CU.
    if (kn.wx4_persist && nrep == 3 && wx4p_ok && tiles(s.n, s.h, s.w, 16) * groups >= (long)kn.wx4_persist_min * n_cu && rows_pin != 8)
      return p.add(VIRNET_LAUNCH_WX4P, 16, 1, nrep, 0, slab_base, groups, 1);
    return p.add(VIRNET_LAUNCH_WX4, 16, 1, nrep, 0, slab_base, groups);
  };
  // 160 channels (SISR level 1): five slabs in ONE launch of the 8-row form with one workgroup per CU (conv_f16_wx4h.hip, NREP = 5) instead
  // of 3 + 2 slabs in two launches that each stage and transform the pixel tile.  VIRNET_WX4_WIDE=0: the two launches.
  if (nb == 5 && rows_pin != 16 && !emit_rows && !kn.wx4_wide_off && !kn.wx4_nrep_set) return one(5, 0, 1);
  if (int rc = one(3, 0, g.n3)) return rc;
  if (int rc = one(2, 3 * g.n3, g.n2)) return rc;
  return one(1, 3 * g.n3 + 2 * g.n2, g.n1);
}

// ---- virnet_conv_wx4x1 (conv_f16_wx4x1.hip): the one-product form has ONE tile form -- 16-row tiles, 8 waves, one workgroup per CU -- so
// the plan is the slab grouping alone: 3 where the count allows, the remainder in 2s, a lone odd slab by itself (slab_groups); launches
// that leave CUs empty take the smallest slab count per workgroup that still fits one round (plan_wx4's rule on 16-row tiles).
// VIRNET_WX4_NREP pins the grouping as it does for virnet_conv_wx4.  No result bit depends on the grouping.
inline int plan_wx4x1(const ConvShape& s, const ConvKnobs& kn, int n_cu, ConvPlan& p) {
  const int nb = s.nb;
  SlabGroups g = slab_groups(nb);
  int want = kn.wx4_nrep;
  if (want == 0) {
    const long t16 = tiles(s.n, s.h, s.w, 16);
    if (t16 * (g.n3 + g.n2 + g.n1) < n_cu) {
      for (int c = 1; c <= 2 && want == 0; ++c)
        if (nb % c == 0 && t16 * (nb / c) <= n_cu) want = c;
    }
  }
  if (want == 1) g = {0, 0, nb};
  else if (want == 2) g = {0, nb / 2, nb - 2 * (nb / 2)};
  if (int rc = p.add(VIRNET_LAUNCH_WX4X1, 16, 1, 3, 0, 0, g.n3)) return rc;
  if (int rc = p.add(VIRNET_LAUNCH_WX4X1, 16, 1, 2, 0, 3 * g.n3, g.n2)) return rc;
  return p.add(VIRNET_LAUNCH_WX4X1, 16, 1, 1, 0, 3 * g.n3 + 2 * g.n2, g.n1);
}

// ---- virnet_conv_f16, stride 1 (conv_f16.hip) --------------------------------------------------------------------------------
// variant = MREP: 8-row (2) or 4-row (1) tiles.  planar: the NCHW store (one slab); emit: T emission (8-row tiles whatever the grid)
inline int plan_f16(const ConvShape& s, bool planar, bool emit, const ConvKnobs& kn, ConvPlan& p) {
  const int nb = s.nb, forced_m = kn.f16_mrep;
  const long tiles8 = tiles(s.n, s.h, s.w, 8);
  auto mrep_of = [&](int groups) { return (forced_m == 1 || forced_m == 2) ? forced_m : (tiles8 * groups >= 1024 ? 2 : 1); };
  if (planar) { const int m = mrep_of(1); return p.add(VIRNET_LAUNCH_F16, 4 * m, 1, 1, m, 0, 1); }
  SlabGroups g = slab_groups(nb);
  // Launches far from filling the chip (deep levels of single images: a 64x64 x 288-channel conv is 32 tiles x 3 channel blocks = 96
  // workgroups of 18 chunks each): one slab per workgroup triples the grid, shortens every workgroup and puts channel counts that are
  // not multiples of 96 (160 = 3 + 2, 224 = 3 + 2 + 2) into ONE launch.  No result bit depends on the grouping.  VIRNET_F16_SPLIT_WGS:
  // the largest 3-slab grid that is split (0 = never).
  // A MIXED grouping (160 = 3 + 2 slabs) is two launches one after the other, each on half of the chip when it has ~128 workgroups:
  // there the split pays up to twice the grid (SISR x4, one image, 160-channel level: 2 x 128 workgroups in 58 us -> 640 in ~30;
  // the forward 1.21 -> 1.08 ms, profiles/r05_probes.md 11)
  const bool mixed = (g.n3 > 0) + (g.n2 > 0) + (g.n1 > 0) >= 2;
  const long split_below = kn.f16_split_set ? kn.f16_split_wgs : (mixed ? 256 : 128);
  if (nb > 1 && tiles(s.n, s.h, s.w, 4) * (g.n3 + g.n2 + g.n1) <= split_below && !emit) g = {0, 0, nb};
  auto one = [&](int nrep, int slab_base, int groups) -> int {
    const int m = emit ? 2 : mrep_of(groups);
    return p.add(VIRNET_LAUNCH_F16, 4 * m, 1, nrep, m, slab_base, groups);
  };
  if (int rc = one(3, 0, g.n3)) return rc;
  if (int rc = one(2, 3 * g.n3, g.n2)) return rc;
  return one(1, 3 * g.n3 + 2 * g.n2, g.n1);
}

// ---- virnet_conv_f16, stride 2 (conv_f16_s2.hip); s.h / s.w = OUTPUT size ----------------------------------------------------------
inline int plan_f16_s2(const ConvShape& s, const ConvKnobs& kn, ConvPlan& p) {
  const int nb = s.nb;
  const long tiles4 = tiles(s.n, s.h, s.w, 4);
  // 160 and 224 channels (SISR: 5 / 7 slabs) as ONE 4-wave launch with 5 / 7 slabs per workgroup (the pixel tile staged once) instead of
  // 3 + 2 / 3 + 2 + 2: the workgroup is alone on its CU either way (75 KB pixel tiles), so its 512 registers per wave are there
  // ... unless the launch is a few dozen tiles (SISR, one image: 160 -> 224 channels onto 64 x 64 = 32 tiles = 32 workgroups on 256 CUs,
  // 54 us): then one slab per workgroup, all slabs in ONE launch (32 x 7 = 224 workgroups).  VIRNET_S2_SPLIT_TILES: the largest such launch.
  if (nb > 1 && tiles4 <= kn.s2_split_tiles) return p.add(VIRNET_LAUNCH_S2, 4, 1, 1, 0, 0, nb);
  if ((nb == 5 || nb == 7 || nb == 4) && !kn.s2_wide_off) return p.add(VIRNET_LAUNCH_S2, 4, 1, nb, 0, 0, 1);
  // Small launches (single images): with 6 slabs per workgroup a 64x64 output is 32 workgroups on a 256-CU chip (and 288 channels two
  // such launches back to back: 48 + 36 us measured); 3-slab workgroups triple the grid and put all slabs in ONE launch.  The slab
  // grouping does not change any result bit (channels are independent).
  const int n6 = nb / 6;
  return add_groups6(p, VIRNET_LAUNCH_S2, 4, 0, slab_groups6(nb, n6 > 0 && tiles4 * n6 < 192 ? 3 : 6));
}

// ---- virnet_conv_f16, transposed 2x2 / stride 2 (conv_f16_pw.hip); s.nb = 4 * cout / 32 ----------------------------------------------
// padded contraction length of the weight image: the kernel walks K in stages of two 16-channel chunks when the channel count allows
// (two workgroups per CU), of three otherwise
inline int convt_kpad(int cin) { return cin % 32 == 0 ? cin : (cin + 47) / 48 * 48; }
// pointwise: 128-pixel tiles, rows = 0.  variant = KS, chunks per stage: 2 / two workgroups per CU when the padded contraction length allows (VIRNET_CONVT_KS=3: round 2's form)
inline int plan_f16_convt(const ConvShape& s, int cin, const ConvKnobs& kn, ConvPlan& p) {
  const int kpad = convt_kpad(cin);
  const bool ks2 = kpad % 32 == 0 && !(kn.convt_ks3 && kpad % 48 == 0);
  return add_groups6(p, VIRNET_LAUNCH_CONVT, 0, ks2 ? 2 : 3, slab_groups6(s.nb, kn.convt_slabs));
}

}  // namespace virnet
