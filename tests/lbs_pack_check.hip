// Stand-alone check of the model packing (egogen_amd/csrc/lbs_pack.hip): host code only, needs no GPU, is not loaded into Python.
//
//   lbs_pack_check              packs the built-in models and the error cases, prints one line per packed array (count + FNV-1a hash),
//                               per scalar, the vertex permutation and the PoseConsts band fields (fp32 bit patterns)
//   lbs_pack_check raw FILE     the same lines for a description stored as a raw file (tests/test_lbs_pack_cpu.py writes one)
//
// The built-in models come from integer formulas - no random generator, no library - so the expected output
// (tests/golden/lbs_pack_check.txt, recorded from the code before the packing was split off, see profiles/lbs_pack.md) depends on
// nothing but the packing.  Between them the models reach every branch of the packing; the program asserts that each was reached.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../egogen_amd/csrc/lbs_pack.h"

static std::string g_error;
void egx_set_error(const std::string& msg) { g_error = msg; }

#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      fprintf(stderr, "lbs_pack_check: %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                               \
    }                                                                        \
  } while (0)

namespace {

struct Model {   // owns the tables of a description
  int V = 0;
  std::vector<float> vt, sd, pd, jr, w, hcl, hcr, hml, hmr, bary;
  std::vector<int32_t> parents, extra, lmk, marker, feet;
  egx_body_model_host desc() const {
    egx_body_model_host d;
    d.num_verts = V;
    d.v_template_host = vt.data(); d.shapedirs_host = sd.data(); d.posedirs_host = pd.data(); d.J_regressor_host = jr.data();
    d.parents_host = parents.data(); d.lbs_weights_host = w.data();
    d.hand_comps_l_host = hcl.data(); d.hand_comps_r_host = hcr.data(); d.hand_mean_l_host = hml.data(); d.hand_mean_r_host = hmr.data();
    d.extra_vids_host = extra.data(); d.lmk_vids_host = lmk.data(); d.lmk_bary_host = bary.data();
    d.num_markers = (int)marker.size(); d.marker_vids_host = marker.data();
    d.num_feet = (int)feet.size(); d.feet_vids_host = feet.data();
    return d;
  }
};

// a value in [-1, 1) with 16 significant bits, exact in fp32, from an index and a stream number
float unit(uint32_t i, uint32_t stream) {
  const uint32_t h = (i * 2654435761u + stream * 40503u) * 2246822519u;
  return ((float)((h >> 12) & 0xffffu) - 32768.f) / 32768.f;
}

// Common part of the built-in models: a body of V vertices around a 55-joint chain; `blend` scales the blend shapes (metres).
Model base_model(int V, float blend) {
  Model m;
  m.V = V;
  m.vt.resize((size_t)V * 3); m.sd.resize((size_t)V * 30); m.pd.resize((size_t)486 * 3 * V); m.jr.assign((size_t)55 * V, 0.f);
  m.w.assign((size_t)V * 55, 0.f);
  for (size_t i = 0; i < m.vt.size(); ++i) m.vt[i] = unit((uint32_t)i, 1) * 0.75f;
  for (size_t i = 0; i < m.sd.size(); ++i) m.sd[i] = unit((uint32_t)i, 2) * blend;
  for (size_t i = 0; i < m.pd.size(); ++i) m.pd[i] = unit((uint32_t)i, 3) * blend * 0.5f;
  for (int j = 0; j < 55; ++j)
    for (int t = 0; t < 4; ++t) m.jr[(size_t)j * V + (j * 3 + t * 5) % V] += 0.25f;
  m.parents.resize(55);
  for (int j = 0; j < 55; ++j) m.parents[j] = j == 0 ? -1 : (j - 1) / 2;
  m.hcl.resize(540); m.hcr.resize(540); m.hml.resize(45); m.hmr.resize(45); m.bary.resize(153);
  for (int i = 0; i < 540; ++i) { m.hcl[i] = unit(i, 4) * 0.125f; m.hcr[i] = unit(i, 5) * 0.125f; }
  for (int i = 0; i < 45; ++i) { m.hml[i] = unit(i, 6) * 0.0625f; m.hmr[i] = unit(i, 7) * 0.0625f; }
  for (int i = 0; i < 51; ++i) { m.bary[3 * i] = 0.5f; m.bary[3 * i + 1] = 0.25f + (i % 4) / 32.f; m.bary[3 * i + 2] = 0.25f - (i % 4) / 32.f; }
  return m;
}

// two joints per vertex, weights k/8 + (8 - k)/8: a convex combination whose fp32 sum is exactly 1
void bind(Model& m, int v, int ja, int jb, int k) {
  m.w[(size_t)v * 55 + ja] = k / 8.f;
  m.w[(size_t)v * 55 + jb] = (8 - k) / 8.f;
}

// id tables over the `npick` vertices first + stride * i: 25 markers, 21 extra, 153 landmark corners, ids repeat between the tables
void pick_tables(Model& m, int first, int stride, int npick) {
  m.marker.resize(25); m.extra.resize(21); m.lmk.resize(153);
  for (int i = 0; i < 25; ++i) m.marker[i] = first + stride * ((i * 5) % npick);
  for (int i = 0; i < 21; ++i) m.extra[i] = first + stride * ((i * 3 + 1) % npick);
  for (int i = 0; i < 153; ++i) m.lmk[i] = first + stride * (i % npick);
}

// Model "tiles": V = 200 (7 tiles, 24 padding rows).  In the packed order: 64 picked vertices (two tiles) | 32 vertices without any
// weight (a tile with the single zero entry) | 32 feet vertices bound to joint 0 alone (a tile outside the SDF list) | 72 vertices
// bound to two joints each out of many (tiles whose joint list needs two skinning k-steps).  Not convex.
Model model_tiles() {
  Model m = base_model(200, 1.f / 128);
  pick_tables(m, 2, 3, 64);                                                   // picked: 2, 5, 8, .. 191
  int other = 0;
  for (int v = 0; v < 200; ++v) {
    const bool picked = v % 3 == 2 && v < 192;
    if (picked) bind(m, v, 1 + v % 7, 20 + v % 5, 1 + v % 7);
    else if (other < 32) ++other;                                             // no weight
    else if (other < 64) { m.w[(size_t)v * 55] = 1.f; m.feet.push_back(v); ++other; }
    else { bind(m, v, 1 + (other * 7) % 25, 26 + (other * 11) % 29, 1 + other % 7); ++other; }
  }
  return m;
}

// Model "convex": V = 96, convex weights, blend shapes of a fraction of a millimetre: passes the reference margin (cull_ok = 1).
// `blend` = 1/16 gives the model that is convex but fails the margin; `negative` the one with a negative weight.
Model model_convex(float blend, bool negative) {
  Model m = base_model(96, blend);
  pick_tables(m, 0, 2, 40);
  for (int v = 0; v < 96; ++v) bind(m, v, v / 8, 20 + 2 * (v / 8), 1 + v % 7);
  for (int i = 0; i < 12; ++i) m.feet.push_back(95 - 2 * i);
  if (negative) { m.w[(size_t)50 * 55 + 3] = 1.25f; m.w[(size_t)50 * 55 + 4] = -0.25f; for (int j = 0; j < 55; ++j) if (j != 3 && j != 4) m.w[(size_t)50 * 55 + j] = 0.f; }
  return m;
}

uint64_t fnv(const void* p, size_t n) {
  const unsigned char* b = static_cast<const unsigned char*>(p);
  uint64_t h = 1469598103934665603ull;
  for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
  return h;
}
template <typename T>
void line(const char* model, const char* name, const std::vector<T>& v) {
  printf("%s.%s %zu %016llx\n", model, name, v.size(), (unsigned long long)fnv(v.data(), v.size() * sizeof(T)));
}
void bits(const char* model, const char* name, const float* f, int n) {
  printf("%s.%s", model, name);
  for (int i = 0; i < n; ++i) { uint32_t u; memcpy(&u, f + i, 4); printf(" %08x", u); }
  printf("\n");
}

void print_packed(const char* n, const egx_body_model_host& d, const LbsPacked& p) {
  printf("%s.sizes V=%d NVT=%d NW=%d M=%d NP=%d verts_pick_tiles=%d verts_sdf_tiles=%d cull_ok=%d sdf_lead_picks=%d\n", n, p.V, p.NVT, p.NW,
         p.M, p.NP, p.verts_pick_tiles, p.verts_sdf_tiles, p.cull_ok, p.sdf_lead_picks);
  bits(n, "rest_pelvis", p.rest_pelvis, 3);
  bits(n, "cull_ref_margin", &p.cull_ref_margin, 1);
  line(n, "perm", p.perm); line(n, "dirs", p.dirs); line(n, "dirs_rm", p.dirs_rm); line(n, "dirs3", p.dirs3); line(n, "dirs4", p.dirs4);
  line(n, "tj_off", p.tj_off); line(n, "tj_idx", p.tj_idx); line(n, "tj_w", p.tj_w); line(n, "skin_ks_off", p.skin_ks_off);
  line(n, "skinW", p.skinW); line(n, "pick_slot", p.pick_slot); line(n, "marker_slot", p.marker_slot); line(n, "extra_slot", p.extra_slot);
  line(n, "lmk_slot", p.lmk_slot); line(n, "lmk_bary", p.lmk_bary); line(n, "pick_tiles", p.pick_tiles); line(n, "sdf_tiles", p.sdf_tiles);
  line(n, "vflags", p.vflags); line(n, "pc", p.pc); line(n, "cull_E", p.cull_E); line(n, "cull_D0", p.cull_D0);
  printf("%s.permutation", n);
  for (int v : p.perm) printf(" %d", v);
  printf("\n");
  const PoseConsts& pc = p.pc[0];
  bits(n, "band.fix_c", pc.fix_c, NJ); bits(n, "band.fix_d", pc.fix_d, NJ); bits(n, "band.fix_pf", &pc.fix_pf, 1);
  bits(n, "band.fix_dpf", &pc.fix_dpf, 1); bits(n, "band.shape_c", pc.shape_c, 10); bits(n, "band.vt_max", &pc.vt_max, 1);
  bits(n, "band.w_abs_max", &pc.w_abs_max, 1);
  // the tables the point sets share with the model (egx_point_set_create)
  std::vector<float> Jt(NJ * 3), Jsd(NJ * 30);
  lbs_fold_joint_regressor(&d, Jt.data(), Jsd.data());
  line(n, "fold.Jt", Jt); line(n, "fold.Jsd", Jsd);
}

// which branches of the packing a packed model reached
enum { PADDING, TWO_KSTEPS, ZERO_ENTRY, FEET_TILE, PICKS_SPREAD, SLOTS_REUSED, CULL_OK, NEGATIVE_WEIGHT, MARGIN_FAILS, N_BRANCHES };
void branches(const egx_body_model_host& d, const LbsPacked& p, bool* hit) {
  hit[PADDING] |= p.V % 32 != 0 && p.perm.back() == -1;
  for (int vt = 0; vt < p.NVT; ++vt) {
    hit[TWO_KSTEPS] |= p.tj_off[vt + 1] - p.tj_off[vt] > 8 && p.skin_ks_off[vt + 1] - p.skin_ks_off[vt] >= 2;
    bool none = p.tj_off[vt + 1] - p.tj_off[vt] == 1 && p.tj_idx[p.tj_off[vt]] == 0;
    for (int r = 0; r < 32 && none; ++r) none = p.tj_w[(size_t)p.tj_off[vt] * 32 + r] == 0.f;
    hit[ZERO_ENTRY] |= none;
  }
  hit[FEET_TILE] |= (int)p.sdf_tiles.size() < p.NVT;
  hit[PICKS_SPREAD] |= p.pick_tiles.size() > 1;
  hit[SLOTS_REUSED] |= p.NP < p.M + NEXTRA + NLMK * 3;
  bool negative = false;
  for (size_t i = 0; i < (size_t)p.V * NJ; ++i) negative |= d.lbs_weights_host[i] < 0.f;
  hit[CULL_OK] |= p.cull_ok == 1 && p.cull_ref_margin > 0.f && p.cull_ref_margin <= 0.15f;
  hit[NEGATIVE_WEIGHT] |= negative && p.cull_ok == 0 && p.cull_ref_margin == 0.f;
  hit[MARGIN_FAILS] |= !negative && p.cull_ok == 0 && p.cull_ref_margin > 0.15f;
}

void pack_and_print(const char* name, const Model& m, bool* hit) {
  const egx_body_model_host d = m.desc();
  LbsPacked p;
  CHECK(lbs_pack_model(&d, &p) == EGX_OK);
  print_packed(name, d, p);
  if (hit) branches(d, p, hit);
}

// an error return: EGX_ERR_ARG, its message, and nothing packed
void expect_error(const char* name, const egx_body_model_host& d) {
  LbsPacked p;
  g_error.clear();
  const int rc = lbs_pack_model(&d, &p);
  CHECK(rc == EGX_ERR_ARG);
  CHECK(p.V == 0 && p.perm.empty() && p.dirs.empty() && p.pc.empty() && p.tj_idx.empty());
  printf("error.%s rc=%d %s\n", name, rc, g_error.c_str());
}

void error_cases() {
  const Model good = model_convex(1.f / 4096, false);
  { Model m = good; m.marker[3] = m.V; expect_error("marker_id", m.desc()); }
  { Model m = good; m.extra[20] = -1; expect_error("extra_id", m.desc()); }
  { Model m = good; m.lmk[152] = m.V + 5; expect_error("landmark_id", m.desc()); }
  { Model m = good; m.feet[0] = m.V; expect_error("feet_id", m.desc()); }
  { Model m = good; m.parents[5] = 7; expect_error("parents", m.desc()); }
  { egx_body_model_host d = good.desc(); d.shapedirs_host = nullptr; expect_error("null_table", d); }
}

template <typename T>
void read_into(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  CHECK(fread(v.data(), sizeof(T), n, f) == n);
}

// raw file: int32 V, M, num_feet, then the tables of egx_body_model_host in the order of the struct's fields, markers and feet last
Model read_raw(const char* path) {
  FILE* f = fopen(path, "rb");
  CHECK(f);
  int32_t h[3];
  CHECK(fread(h, 4, 3, f) == 3);
  Model m;
  const size_t V = (size_t)(m.V = h[0]);
  read_into(f, m.vt, V * 3); read_into(f, m.sd, V * 30); read_into(f, m.pd, 486 * 3 * V); read_into(f, m.jr, 55 * V);
  read_into(f, m.parents, 55); read_into(f, m.w, V * 55); read_into(f, m.hcl, 540); read_into(f, m.hcr, 540); read_into(f, m.hml, 45);
  read_into(f, m.hmr, 45); read_into(f, m.extra, 21); read_into(f, m.lmk, 153); read_into(f, m.bary, 153);
  read_into(f, m.marker, (size_t)h[1]); read_into(f, m.feet, (size_t)h[2]);
  CHECK(fgetc(f) == EOF);
  fclose(f);
  return m;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 3 && std::string(argv[1]) == "raw") {
    pack_and_print("raw", read_raw(argv[2]), nullptr);
    return 0;
  }
  CHECK(argc == 1);
  bool hit[N_BRANCHES] = {};
  pack_and_print("tiles", model_tiles(), hit);
  CHECK(hit[PADDING] && hit[TWO_KSTEPS] && hit[ZERO_ENTRY] && hit[FEET_TILE] && hit[PICKS_SPREAD] && hit[SLOTS_REUSED]);
  pack_and_print("convex", model_convex(1.f / 4096, false), hit);
  CHECK(hit[CULL_OK]);
  pack_and_print("negative", model_convex(1.f / 4096, true), hit);
  CHECK(hit[NEGATIVE_WEIGHT]);
  pack_and_print("margin", model_convex(1.f / 16, false), hit);
  CHECK(hit[MARGIN_FAILS]);
  error_cases();
  return 0;
}
