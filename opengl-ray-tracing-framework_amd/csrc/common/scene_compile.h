// scene_compile.h — the scene compiler: the caller's scene description (rt_scene_soa, or the
// reference's own AoS encodings) -> the device layout, as bytes ready to upload (host side).
//
// Plain C++17, no HIP: rt_render.hip includes it for the product (rt_set_scene uploads what
// compile() returns), and librtscene.so exports it (rts_compile_scene, include/rt_scene.h) so CPU
// tests call the same code.  What is decided here: the validation of the caller's tree, the
// children-in-parent binary nodes, the leaf ranks, the 4-wide tree (whether traversal reaches
// exactly the reference's leaves, whether a Q_EMPTY slot can ever be entered) and the culling
// bound (whether culling is exact).
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <functional>
#include <string>
#include <utility>
#include <vector>

#include "glsl_math.h"
#include "rt_abi.h"
#include "tri_filter.h"

namespace scn {

#define SCN_HD TRIF_HD

// Child references of both trees: an internal node's index, or a leaf's triangle range
// (LEAF_BIT | first << 4 | count - 1, at most 16 triangles); Q_EMPTY marks an empty 4-wide slot.
constexpr int Q_EMPTY = 0x7fffffff;
constexpr uint32_t LEAF_BIT = 0x80000000u;
constexpr bool ref_is_leaf(int r) { return ((uint32_t)r & LEAF_BIT) != 0u; }
constexpr int leaf_first(int r) { return (int)(((uint32_t)r & 0x7fffffffu) >> 4); }
constexpr int leaf_count(int r) { return (int)((uint32_t)r & 15u) + 1; }
constexpr int leaf_ref(int first, int n) { return (int)(LEAF_BIT | ((uint32_t)first << 4) | (uint32_t)(n - 1)); }

// The traversal-structure variants (the release library always takes the defaults)
struct Options {
  bool rebuild = true;   // internal levels rebuilt over the reference's leaves (false: the reference's own)
  bool greedy = false;   // 4-wide collapse: largest area first instead of the SAH-optimal one
  bool bfs = true;       // 4-wide nodes numbered breadth-first (false: depth-first)
  bool wide = true;      // false: binary traversal only
};

// Binary node, the layout of rtd::GNode (rt_device.h): left box lo.xyz hi.xyz, right box lo.xyz
// hi.xyz, then left ref, right ref, rank of the first leaf of the right subtree, -
struct BNode {
  float box[12];
  int32_t ref[4];
};
// 4-wide node, the layout of rtd::QNode: lo[axis][slot], hi[axis][slot], the slots' refs
struct WNode {
  float lo[3][4], hi[3][4];
  int32_t ref[4], pad[4];
};
static_assert(sizeof(BNode) == 64 && sizeof(WNode) == 128, "device record sizes");

struct Compiled {
  // 4 floats per texel: tri {p, Ng.k}, trx the traversal records (tri_filter.h), trin {n, material
  // id / leaf rank / 0}, hrec the shade's hit records; mats 32 floats per material
  std::vector<float> tri, trx, trin, hrec, mats;
  std::vector<BNode> nodes;
  std::vector<WNode> qnodes;
  std::vector<int32_t> tri_mat;  // the per-triangle material ids
  int n_tri = 0, n_mats = 0;
  int root = 0, has_scene = 0, depth = 1, qroot = 0, qdepth = 1;
  bool wide = false;  // 4-wide traversal available for this scene
  double cull_R = 0.0, cull_K = 0.0, cull_off = 0.0;  // culling bound of the scene (cull_bound_stats)
  double tri_k1 = 0.0, tri_k0 = 0.0;                  // the edge filter's margin
  int tri_flagged = 0;
  // the edge filter's state (trif::Consts): the caps of the last compile and the extrema k1, k0 are
  // formed from; update_geometry keeps the caps and lets the extrema grow
  double s_cap = 0.0, sc_cap = 0.0, s_max = 0.0, sc_max = 0.0, c_min = 1.0;
  bool qbuilt = false;  // qnodes / qroot describe a 4-wide tree (build_wide did not give up)
};

// Same fp32 operations as the shader's per-test N = normalize(cross(p2-p1, p3-p1)) (RT:253).
SCN_HD inline void geometric_normal(const float* p1, const float* p2, const float* p3, float* n) {
  float ax = p2[0] - p1[0], ay = p2[1] - p1[1], az = p2[2] - p1[2];
  float bx = p3[0] - p1[0], by = p3[1] - p1[1], bz = p3[2] - p1[2];
  float cx = ay * bz - by * az, cy = az * bx - bz * ax, cz = ax * by - bx * ay;
  float inv = 1.0f / sqrtf(cx * cx + cy * cy + cz * cz);
  n[0] = cx * inv; n[1] = cy * inv; n[2] = cz * inv;
}

// Culling bound ("What the culling margin covers").  A subtree may be skipped when
// its box entry t0 exceeds the best hit; that is exact only if no triangle inside the box can be
// accepted by the reference's test (RT:241-299) at a computed t below t0.  An accepted hit point
// P = S + d*t (fp32) lies within eps (per axis) of its triangle, hence of every box holding it:
//   off-plane |(P - p1).N| <= 36 u R  (rounding of RT:265 and of P; R bounds |coords|, origins),
//   in-plane slack of the three edge signs <= 70 u R / cos(theta)  (theta: fp32 N vs exact normal),
//   X = S + d*t (exact) vs P: <= 8 u R,
//   + the triangle's vertices off the plane (p1, N): max_k |(pk - p1).N|,
// so t >= t0 - eps * max|1/d_a|.  Returned per scene: K (units of u R) and off; the render
// doubles eps = K u R + off as safety.  Degenerate (zero-area with a finite fp32 normal) or badly
// conditioned triangles, triangles outside their leaf box, or a caller's box that does not lie
// inside its parent's (compile()), give K = inf: no culling.
struct CullStats {
  double R = 0.0, K = 0.0, off = 0.0;
};
// One triangle's contribution; the scene's three values are the maxima over its triangles.
SCN_HD inline CullStats cull_tri(const float* p1, const float* p2, const float* p3) {
  CullStats cs;
  const float* p[3] = {p1, p2, p3};
  float ng[3];
  geometric_normal(p[0], p[1], p[2], ng);
  for (int k = 0; k < 3; k++)
    for (int a = 0; a < 3; a++) cs.R = trif::dmax_(cs.R, fabs((double)p[k][a]));
  if (!(trif::finitef_(ng[0]) && trif::finitef_(ng[1]) && trif::finitef_(ng[2]))) return cs;  // never hit (NaN tests)
  double e1[3], e2[3], cx[3];
  for (int a = 0; a < 3; a++) { e1[a] = (double)p[1][a] - p[0][a]; e2[a] = (double)p[2][a] - p[0][a]; }
  cx[0] = e1[1] * e2[2] - e1[2] * e2[1];
  cx[1] = e1[2] * e2[0] - e1[0] * e2[2];
  cx[2] = e1[0] * e2[1] - e1[1] * e2[0];
  const double nrm = sqrt(cx[0] * cx[0] + cx[1] * cx[1] + cx[2] * cx[2]);
  const double cosT = nrm > 0.0 ? (ng[0] * cx[0] + ng[1] * cx[1] + ng[2] * cx[2]) / nrm : 0.0;
  if (!(cosT > 0.25)) { cs.K = (double)INFINITY; return cs; }
  cs.K = 44.0 + 70.0 / cosT;
  for (int k = 1; k < 3; k++) {
    double o = 0.0;
    for (int a = 0; a < 3; a++) o += ((double)p[k][a] - p[0][a]) * ng[a];
    cs.off = trif::dmax_(cs.off, fabs(o));
  }
  return cs;
}
inline void cull_merge(CullStats& cs, const CullStats& t) {
  cs.R = std::max(cs.R, t.R);
  cs.K = std::max(cs.K, t.K);
  cs.off = std::max(cs.off, t.off);
}
inline CullStats cull_bound_stats(const rt_scene_soa* s) {
  CullStats cs;
  const int nt = s->n_triangles;
  for (int i = 0; i < nt; i++) cull_merge(cs, cull_tri(s->p1 + 3 * i, s->p2 + 3 * i, s->p3 + 3 * i));
  // every leaf's triangles inside the leaf's box (the reference's own boxes are their min/max)
  for (int n = 1; n < s->n_nodes && s->node_n; n++) {
    if (s->node_n[n] <= 0) continue;
    for (int i = s->node_index[n]; i < s->node_index[n] + s->node_n[n] && i < nt; i++)
      for (const float* q : {s->p1 + 3 * i, s->p2 + 3 * i, s->p3 + 3 * i})
        for (int a = 0; a < 3; a++)
          if (!(q[a] >= s->node_aa[3 * n + a] && q[a] <= s->node_bb[3 * n + a])) cs.K = INFINITY;
  }
  return cs;
}

// Material.h fields -> 32-float device entry; ax/ay by getMaterial's formula (RT:205-207).
inline void pack_material(const rt_material& m, float* o) {
  const float* f = reinterpret_cast<const float*>(&m);
  for (int k = 0; k < 24; k++) o[k] = f[k];
  float aspect = gm::sqrt_(1.0f - m.anisotropic * 0.9f);
  o[24] = gm::max_(0.001f, (m.roughness * m.roughness) / aspect);
  o[25] = gm::max_(0.001f, (m.roughness * m.roughness) * aspect);
  int mt = (int)m.medium_type;
  memcpy(&o[26], &mt, 4);
  o[27] = o[28] = o[29] = o[30] = o[31] = 0.0f;
}

// New internal levels over the reference's leaves.  A leaf keeps its triangle range and its exact
// box (the reference's, RT:363-368); every internal box is the exact min/max union of the boxes
// below it.  The slab arithmetic is monotone in the box planes, so a box can only be hit when
// every box above it is: the traversal reaches exactly the leaves whose own box the reference's
// ray hits, whatever the internal levels are (the reference's exact-tie order is kept separately,
// by the leaf ranks of its own tree).  The reference reaches those same leaves only if each of
// the caller's tested boxes lies inside its parent's; compile() checks that and keeps a tree
// that does not nest on the binary traversal.  The reference's top levels are X-median splits (R18: SAH
// costs above INF = 114514 fall back to the median), so a full-sweep SAH over the leaf boxes
// (centroid order per axis, cost = area x triangles) gives a tree with fewer node visits.
// Returns the root of `out` (binary nodes, host only: the device keeps the reference tree).
inline int rebuild_over_leaves(const std::vector<BNode>& gn, int root, std::vector<BNode>& out) {
  struct Box {
    float lo[3], hi[3];
  };
  struct Prim {
    int ref, n;
    Box b;
    double c[3];
  };
  std::vector<Prim> prims;
  std::vector<int> st{root};
  while (!st.empty()) {
    const BNode g = gn[st.back()];
    st.pop_back();
    const Box bl = {{g.box[0], g.box[1], g.box[2]}, {g.box[3], g.box[4], g.box[5]}};
    const Box br = {{g.box[6], g.box[7], g.box[8]}, {g.box[9], g.box[10], g.box[11]}};
    const int refs[2] = {g.ref[0], g.ref[1]};
    const Box* boxes[2] = {&bl, &br};
    for (int k = 0; k < 2; k++) {
      if (!ref_is_leaf(refs[k])) { st.push_back(refs[k]); continue; }
      Prim p;
      p.ref = refs[k];
      p.n = leaf_count(refs[k]);
      p.b = *boxes[k];
      for (int a = 0; a < 3; a++) p.c[a] = 0.5 * ((double)p.b.lo[a] + (double)p.b.hi[a]);
      prims.push_back(p);
    }
  }
  auto unite = [](const Box& a, const Box& b) {
    Box u;
    for (int k = 0; k < 3; k++) { u.lo[k] = std::min(a.lo[k], b.lo[k]); u.hi[k] = std::max(a.hi[k], b.hi[k]); }
    return u;
  };
  auto area = [](const Box& b) {
    double e[3];
    for (int k = 0; k < 3; k++) e[k] = std::max(0.0, (double)b.hi[k] - (double)b.lo[k]);
    return e[0] * e[1] + e[1] * e[2] + e[2] * e[0];
  };
  std::vector<int> idx(prims.size()), tmp(prims.size());
  for (size_t i = 0; i < idx.size(); i++) idx[i] = (int)i;
  std::vector<double> right_cost(prims.size() + 1);
  out.clear();
  out.reserve(prims.size());
  std::function<int(int, int, Box&)> rec = [&](int b, int e, Box& box) -> int {
    if (e - b == 1) {
      box = prims[idx[b]].b;
      return prims[idx[b]].ref;
    }
    double best = 1e300;
    int bax = 0, bpos = b + (e - b) / 2;
    for (int ax = 0; ax < 3; ax++) {
      std::copy(idx.begin() + b, idx.begin() + e, tmp.begin() + b);
      std::sort(tmp.begin() + b, tmp.begin() + e, [&](int x, int y) {
        return prims[x].c[ax] < prims[y].c[ax] || (prims[x].c[ax] == prims[y].c[ax] && x < y);
      });
      Box acc = prims[tmp[e - 1]].b;
      int cnt = 0;
      for (int i = e - 1; i > b; i--) {  // right_cost[i] = cost of [i, e)
        acc = unite(acc, prims[tmp[i]].b);
        cnt += prims[tmp[i]].n;
        right_cost[i - b] = area(acc) * cnt;
      }
      acc = prims[tmp[b]].b;
      cnt = 0;
      for (int i = b; i < e - 1; i++) {  // split after i: [b, i] | [i + 1, e)
        acc = unite(acc, prims[tmp[i]].b);
        cnt += prims[tmp[i]].n;
        const double c = area(acc) * cnt + right_cost[i + 1 - b];
        if (c < best) { best = c; bax = ax; bpos = i + 1; }
      }
    }
    std::sort(idx.begin() + b, idx.begin() + e, [&](int x, int y) {
      return prims[x].c[bax] < prims[y].c[bax] || (prims[x].c[bax] == prims[y].c[bax] && x < y);
    });
    const int me = (int)out.size();
    out.push_back(BNode{});
    Box lb, rb;
    const int lr = rec(b, bpos, lb), rr = rec(bpos, e, rb);
    out[me] = BNode{{lb.lo[0], lb.lo[1], lb.lo[2], lb.hi[0], lb.hi[1], lb.hi[2],
                     rb.lo[0], rb.lo[1], rb.lo[2], rb.hi[0], rb.hi[1], rb.hi[2]},
                    {lr, rr, 0, 0}};
    box = unite(lb, rb);
    return me;
  };
  Box rootbox;
  return rec(0, (int)prims.size(), rootbox);
}

// Leaf ranks + 4-wide collapse of the binary tree.
// * Leaf rank = position of the leaf in the reference's left-first DFS; gn[k].ref[2] = rank of
//   the first leaf of node k's right subtree; trin[3t+1].w = rank of triangle t's leaf.  These
//   let the 4-wide traversal break exact distance ties the way the reference's visit order does.
// * A WNode replaces a binary node and a cut of its subtree with at most 4 slots, chosen by the
//   SAH-optimal collapse below (or greedily, largest area first).  Boxes are copied bit for bit.
//   A (grand)child box can only be hit when every box above it is (children are min/max over
//   subsets, and the slab arithmetic is monotone), so the 4-wide traversal reaches exactly the
//   reference's leaves.
// Returns false (binary traversal only) when a triangle belongs to two leaves, or when the caller's
// boxes do not nest (`nested` false, compile()): the premise above is then gone.  The leaf ranks
// are written either way.
inline bool build_wide(const Options& opt, std::vector<BNode>& gn, int root, std::vector<float>& trin,
                       std::vector<WNode>& qn, int& qroot, int& qdepth, bool nested = true) {
  const int nt = (int)(trin.size() / 12);
  std::vector<int> tri_rank(nt, -1);
  int rank = 0;
  bool ok = true;
  std::function<void(int)> rank_dfs = [&](int r) {
    if (ref_is_leaf(r)) {
      for (int t = leaf_first(r); t < leaf_first(r) + leaf_count(r); t++) {
        if (tri_rank[t] >= 0) ok = false;
        tri_rank[t] = rank;
      }
      rank++;
      return;
    }
    rank_dfs(gn[r].ref[0]);
    gn[r].ref[2] = rank;
    rank_dfs(gn[r].ref[1]);
  };
  rank_dfs(root);
  for (int t = 0; t < nt; t++) memcpy(&trin[4 * (3 * (size_t)t + 1) + 3], &tri_rank[t], 4);
  if (!ok || !nested) return false;
  // The tree that gets collapsed: by default internal levels rebuilt over the reference's leaves
  // (rebuild_over_leaves), Options::rebuild = false keeps the reference's own internal nodes.
  std::vector<BNode> rebuilt;
  int croot = root;
  const std::vector<BNode>* T = &gn;
  if (!ref_is_leaf(root) && opt.rebuild) {
    croot = rebuild_over_leaves(gn, root, rebuilt);
    T = &rebuilt;
  }
  struct Slot {
    int ref;
    float lo[3], hi[3];
  };
  auto kids = [&](int b, Slot& L, Slot& R) {
    const BNode& g = (*T)[b];
    L = Slot{g.ref[0], {g.box[0], g.box[1], g.box[2]}, {g.box[3], g.box[4], g.box[5]}};
    R = Slot{g.ref[1], {g.box[6], g.box[7], g.box[8]}, {g.box[9], g.box[10], g.box[11]}};
  };
  auto area = [](const Slot& s) {
    double e[3];
    for (int k = 0; k < 3; k++) e[k] = (double)s.hi[k] - (double)s.lo[k];
    return e[0] * e[1] + e[1] * e[2] + e[2] * e[0];
  };
  // Which binary nodes become 4-wide nodes.  Default: the collapse that minimises the summed
  // surface area of the 4-wide nodes (the SAH traversal cost; the leaves and their cost are
  // fixed): f(n, k) = least area of 4-wide roots covering n's subtree with at most k slots,
  // f(n, 1) = A(n) + min_j f(L, j) + f(R, 4 - j), f(n, k) = min(f(n, 1), min_j f(L, j) + f(R, k - j)).
  // Options::greedy: open the largest-area internal slot until there are four.
  const bool greedy = opt.greedy;
  const size_t nb = T->size();
  std::vector<double> f(nb * 5, 0.0);
  std::vector<signed char> split(nb * 5, 0);  // 0: keep the node as one slot, j > 0: j slots to the left
  auto fr = [&](int r, int k) -> double { return ref_is_leaf(r) ? 0.0 : f[(size_t)r * 5 + k]; };
  if (!greedy && !ref_is_leaf(croot)) {
    std::function<void(int)> dp = [&](int b) {
      Slot L, R;
      kids(b, L, R);
      if (!ref_is_leaf(L.ref)) dp(L.ref);
      if (!ref_is_leaf(R.ref)) dp(R.ref);
      Slot U = L;
      for (int k = 0; k < 3; k++) { U.lo[k] = std::min(L.lo[k], R.lo[k]); U.hi[k] = std::max(L.hi[k], R.hi[k]); }
      double open = 1e300;
      int jo = 1;
      for (int j = 1; j <= 3; j++) {
        const double c = fr(L.ref, j) + fr(R.ref, 4 - j);
        if (c < open) { open = c; jo = j; }
      }
      f[(size_t)b * 5 + 1] = area(U) + open;
      split[(size_t)b * 5 + 1] = (signed char)jo;  // the split of the node's own 4-wide record
      for (int k = 2; k <= 4; k++) {
        double best = f[(size_t)b * 5 + 1];
        int bj = 0;
        for (int j = 1; j < k; j++) {
          const double c = fr(L.ref, j) + fr(R.ref, k - j);
          if (c < best) { best = c; bj = j; }
        }
        f[(size_t)b * 5 + k] = best;
        split[(size_t)b * 5 + k] = (signed char)bj;
      }
    };
    dp(croot);
  }
  // DP reconstruction: the slots that binary subtree s contributes when given k of them
  std::function<void(const Slot&, int, std::vector<Slot>&)> collect = [&](const Slot& s, int k, std::vector<Slot>& out) {
    if (ref_is_leaf(s.ref) || k == 1 || split[(size_t)s.ref * 5 + k] == 0) { out.push_back(s); return; }
    const int j = split[(size_t)s.ref * 5 + k];
    Slot L, R;
    kids(s.ref, L, R);
    collect(L, j, out);
    collect(R, k - j, out);
  };
  qdepth = 1;
  std::function<int(int, int)> build = [&](int b, int depth) -> int {
    qdepth = std::max(qdepth, depth);
    const int idx = (int)qn.size();
    qn.push_back(WNode{});
    std::vector<Slot> sl;
    if (greedy) {
      sl.resize(2);
      kids(b, sl[0], sl[1]);
      while (sl.size() < 4) {
        int pick = -1;
        double pa = -1.0;
        for (size_t i = 0; i < sl.size(); i++)
          if (!ref_is_leaf(sl[i].ref) && area(sl[i]) > pa) { pa = area(sl[i]); pick = (int)i; }
        if (pick < 0) break;
        Slot x, y;
        kids(sl[pick].ref, x, y);
        sl[pick] = x;
        sl.insert(sl.begin() + pick + 1, y);
      }
    } else {
      Slot L, R;
      kids(b, L, R);
      const int j = split[(size_t)b * 5 + 1];
      collect(L, j, sl);
      collect(R, 4 - j, sl);
    }
    int refs[4] = {Q_EMPTY, Q_EMPTY, Q_EMPTY, Q_EMPTY};
    for (size_t i = 0; i < sl.size(); i++) refs[i] = ref_is_leaf(sl[i].ref) ? sl[i].ref : build(sl[i].ref, depth + 1);
    // an empty slot is the inverted box lo = +inf, hi = -inf: for a finite 1/d the sign-selected
    // planes give entry t0 = +inf and exit t1 = -inf, so the slab test never hits it (the literal
    // slab of a ray with a zero direction component tests the slot's ref instead: its per-axis
    // min / max would turn the inverted box into an infinite one)
    const float pinf = INFINITY;
    WNode& q = qn[idx];
    for (int k = 0; k < 3; k++)
      for (int i = 0; i < 4; i++) {
        q.lo[k][i] = i < (int)sl.size() ? sl[i].lo[k] : pinf;
        q.hi[k][i] = i < (int)sl.size() ? sl[i].hi[k] : -pinf;
      }
    for (int i = 0; i < 4; i++) q.ref[i] = refs[i];
    return idx;
  };
  qroot = ref_is_leaf(croot) ? croot : build(croot, 1);
  if (!ref_is_leaf(qroot) && opt.bfs) {
    // breadth-first numbering (Options::bfs = false: depth-first): the top levels of the tree are
    // the first nodes (RT_DEBUG_PASSES reports node visits by this index)
    std::vector<int> order{qroot}, newid(qn.size(), -1);
    newid[qroot] = 0;
    for (size_t h = 0; h < order.size(); h++) {
      const WNode& r = qn[order[h]];
      for (int x : r.ref)
        if (x != Q_EMPTY && !ref_is_leaf(x)) {
          newid[x] = (int)order.size();
          order.push_back(x);
        }
    }
    std::vector<WNode> bq(order.size());
    auto remap = [&](int x) { return (x == Q_EMPTY || ref_is_leaf(x)) ? x : newid[x]; };
    for (size_t i = 0; i < order.size(); i++) {
      bq[i] = qn[order[i]];
      for (int32_t& x : bq[i].ref) x = remap(x);
    }
    qn.swap(bq);
    qroot = 0;
  }
  return true;
}

// One triangle's tri texels {p_k, Ng[k]} and the xyz of its trin texels (every .w stays: material
// id, leaf rank, 0).  compile() and the geometry update (host model and device) run this.
SCN_HD inline void tri_record(const float* p1, const float* p2, const float* p3, const float* n1, const float* n2,
                              const float* n3, float* tri, float* trin) {
  float ng[3];
  geometric_normal(p1, p2, p3, ng);
  const float* ps[3] = {p1, p2, p3};
  const float* ns[3] = {n1, n2, n3};
  for (int k = 0; k < 3; k++) {
    float* t = tri + 4 * k;
    float* n = trin + 4 * k;
    t[0] = ps[k][0]; t[1] = ps[k][1]; t[2] = ps[k][2]; t[3] = ng[k];
    n[0] = ns[k][0]; n[1] = ns[k][1]; n[2] = ns[k][2];
  }
}
// The shade's hit record of one triangle: tri's three texels then trin's (floats 24..31 unused)
SCN_HD inline void hit_record(const float* tri, const float* trin, float* hrec) {
  for (int j = 0; j < 12; j++) { hrec[j] = tri[j]; hrec[12 + j] = trin[j]; }
}

// rt_scene_soa -> Compiled.  Returns RT_OK, or RT_ERR_ARG / RT_ERR_LIMIT with the reason in `err`
// and `out` untouched.
inline int compile(const rt_scene_soa* s, const Options& opt, Compiled& out, std::string& err) {
  auto fail = [&](int code, const char* msg) {
    err = msg;
    return code;
  };
  if (s->n_triangles < 0 || s->n_nodes < 0 || s->n_materials < 0) return fail(RT_ERR_ARG, "negative count");
  const int nt = s->n_triangles;
  if (nt > 0 && (!s->p1 || !s->p2 || !s->p3 || !s->n1 || !s->n2 || !s->n3 || !s->material_id || !s->materials))
    return fail(RT_ERR_ARG, "missing triangle arrays");
  if (nt >= (1 << 27)) return fail(RT_ERR_LIMIT, "more than 2^27 triangles");
  for (int i = 0; i < nt; i++)
    if (s->material_id[i] < 0 || s->material_id[i] >= s->n_materials)
      return fail(RT_ERR_ARG, "material_id out of range");
  Compiled c;
  c.n_tri = nt;
  c.n_mats = s->n_materials;
  // ---- triangles
  c.tri.resize(12 * (size_t)nt);
  c.trin.resize(12 * (size_t)nt);
  for (int i = 0; i < nt; i++) {
    float* n = &c.trin[12 * (size_t)i];
    n[3] = n[7] = n[11] = 0.0f;
    memcpy(&n[3], &s->material_id[i], 4);
    tri_record(s->p1 + 3 * i, s->p2 + 3 * i, s->p3 + 3 * i, s->n1 + 3 * i, s->n2 + 3 * i, s->n3 + 3 * i,
               &c.tri[12 * (size_t)i], n);
  }
  // ---- materials
  c.mats.assign(32 * (size_t)std::max(1, s->n_materials), 0.0f);
  for (int m = 0; m < s->n_materials; m++) pack_material(s->materials[m], &c.mats[32 * m]);
  c.tri_mat.assign(s->material_id, s->material_id + nt);
  // ---- BVH: reference numbering -> children-in-parent nodes
  bool nested = true;  // every child's box lies inside its parent's
  if (nt > 0 && s->n_nodes > 1) {
    if (!s->node_left || !s->node_right || !s->node_n || !s->node_index || !s->node_aa || !s->node_bb)
      return fail(RT_ERR_ARG, "missing node arrays");
    const int nn = s->n_nodes;
    std::vector<int> internal_id(nn, -1);
    auto is_leaf = [&](int i) { return s->node_n[i] > 0; };
    auto leaf_of = [&](int i, int& ref) -> int {
      int n = s->node_n[i], first = s->node_index[i];
      if (n > 16) return fail(RT_ERR_LIMIT, "leaf with more than 16 triangles");
      if (first < 0 || first + n > nt) return fail(RT_ERR_ARG, "leaf range outside the triangle list");
      ref = leaf_ref(first, n);
      return RT_OK;
    };
    // DFS from the root (node 1) assigning internal ids, checking structure and depth
    std::vector<std::pair<int, int>> st;
    st.push_back({1, 1});
    std::vector<int> order;
    while (!st.empty()) {
      auto e = st.back();
      st.pop_back();
      int i = e.first;
      if (i <= 0 || i >= nn) return fail(RT_ERR_ARG, "child index out of range");
      c.depth = std::max(c.depth, e.second);
      if (c.depth > 64) return fail(RT_ERR_LIMIT, "BVH deeper than 64 levels");
      if (is_leaf(i)) continue;
      if (internal_id[i] >= 0) return fail(RT_ERR_ARG, "BVH is not a tree");
      if (s->node_left[i] <= 0 || s->node_right[i] <= 0) return fail(RT_ERR_ARG, "internal node without two children");
      internal_id[i] = (int)order.size();
      order.push_back(i);
      st.push_back({s->node_right[i], e.second + 1});
      st.push_back({s->node_left[i], e.second + 1});
    }
    c.nodes.resize(std::max<size_t>(1, order.size()));
    for (size_t k = 0; k < order.size(); k++) {
      int i = order[k];
      int l = s->node_left[i], r = s->node_right[i];
      const float* la = s->node_aa + 3 * l; const float* lb = s->node_bb + 3 * l;
      const float* ra = s->node_aa + 3 * r; const float* rb = s->node_bb + 3 * r;
      // Every tested box inside its parent's (a NaN fails; the root's own box is never tested,
      // RT:338-392): what rebuild_over_leaves, build_wide and the culling bound rest on.
      if (i != 1)
        for (int a = 0; a < 3; a++) {
          const float pa = s->node_aa[3 * i + a], pb = s->node_bb[3 * i + a];
          if (!(la[a] >= pa && lb[a] <= pb && ra[a] >= pa && rb[a] <= pb)) nested = false;
        }
      int lr, rr;
      int rc;
      if (is_leaf(l)) { if ((rc = leaf_of(l, lr))) return rc; } else lr = internal_id[l];
      if (is_leaf(r)) { if ((rc = leaf_of(r, rr))) return rc; } else rr = internal_id[r];
      c.nodes[k] = BNode{{la[0], la[1], la[2], lb[0], lb[1], lb[2], ra[0], ra[1], ra[2], rb[0], rb[1], rb[2]},
                         {lr, rr, 0, 0}};
    }
    if (is_leaf(1)) {
      int rc = leaf_of(1, c.root);
      if (rc) return rc;
    } else {
      c.root = internal_id[1];
    }
    c.has_scene = 1;
  }
  c.qroot = c.root;
  if (c.has_scene) c.wide = c.qbuilt = build_wide(opt, c.nodes, c.root, c.trin, c.qnodes, c.qroot, c.qdepth, nested);
  if (!opt.wide) c.wide = false;
  if (c.nodes.empty()) c.nodes.push_back(BNode{});
  if (c.qnodes.empty()) c.qnodes.push_back(WNode{});
  {  // traversal records: {p1, Ng.x} {R2, Ng.y} {R3, Ng.z} and the edge filter's margin
    c.trx.assign(std::max<size_t>(12, c.tri.size()), 0.0f);
    const trif::Consts k = trif::build(c.tri.data(), nt, c.trx.data());
    c.tri_k1 = k.k1; c.tri_k0 = k.k0; c.tri_flagged = k.flagged;
    c.s_cap = k.s_cap; c.sc_cap = k.sc_cap; c.s_max = k.s_max; c.sc_max = k.sc_max; c.c_min = k.c_min;
  }
  // hit records: tri's three texels then trin's, one 128-B line per triangle
  c.hrec.assign(32 * std::max<size_t>(1, (size_t)nt), 0.0f);
  for (size_t i = 0; i < (size_t)nt; i++) hit_record(&c.tri[12 * i], &c.trin[12 * i], &c.hrec[32 * i]);
  {
    const CullStats cs = cull_bound_stats(s);
    c.cull_R = cs.R; c.cull_K = nested ? cs.K : (double)INFINITY; c.cull_off = cs.off;
  }
  out = std::move(c);
  return RT_OK;
}

// ---- Geometry update: new vertices for some triangles, topology kept ----------
// glm's min / max: the definitions fix which zero a tie between -0 and +0 returns, the same in
// this model, in the device kernels and in the tests.
SCN_HD inline float gmin(float a, float b) { return (b < a) ? b : a; }
SCN_HD inline float gmax(float a, float b) { return (a < b) ? b : a; }

// A leaf's box, the reference's (BVH.h:116-134): from +-1145141919 over its triangles in ascending
// index, per axis the min / max of the three vertices first.  tri: the device layout (12 floats
// per triangle).
SCN_HD inline void leaf_box(const float* tri, int ref, float* lo, float* hi) {
  for (int a = 0; a < 3; a++) { lo[a] = 1145141919.0f; hi[a] = -1145141919.0f; }
  const int first = leaf_first(ref), n = leaf_count(ref);
  for (int t = first; t < first + n; t++) {
    const float* p = tri + 12 * (size_t)t;
    for (int a = 0; a < 3; a++) {
      lo[a] = gmin(lo[a], gmin(p[a], gmin(p[4 + a], p[8 + a])));
      hi[a] = gmax(hi[a], gmax(p[a], gmax(p[4 + a], p[8 + a])));
    }
  }
}
// Box of a binary node: its left child box, then its right one
SCN_HD inline void bnode_box(const BNode& g, float* lo, float* hi) {
  for (int a = 0; a < 3; a++) { lo[a] = gmin(g.box[a], g.box[6 + a]); hi[a] = gmax(g.box[3 + a], g.box[9 + a]); }
}
// Box of a 4-wide node: its non-empty slots in slot order (slot 0 is never empty)
SCN_HD inline void wnode_box(const WNode& q, float* lo, float* hi) {
  for (int a = 0; a < 3; a++) { lo[a] = q.lo[a][0]; hi[a] = q.hi[a][0]; }
  for (int i = 1; i < 4; i++) {
    if (q.ref[i] == Q_EMPTY) continue;
    for (int a = 0; a < 3; a++) { lo[a] = gmin(lo[a], q.lo[a][i]); hi[a] = gmax(hi[a], q.hi[a][i]); }
  }
}

// Every box of both trees from the triangles as they stand.
inline void refit(Compiled& c) {
  if (!c.has_scene) return;
  const float* tri = c.tri.data();
  std::function<void(int, float*, float*)> rb = [&](int ref, float* lo, float* hi) {
    if (ref_is_leaf(ref)) { leaf_box(tri, ref, lo, hi); return; }
    BNode& g = c.nodes[ref];
    rb(g.ref[0], g.box, g.box + 3);
    rb(g.ref[1], g.box + 6, g.box + 9);
    bnode_box(g, lo, hi);
  };
  std::function<void(int, float*, float*)> rw = [&](int ref, float* lo, float* hi) {
    if (ref_is_leaf(ref)) { leaf_box(tri, ref, lo, hi); return; }
    WNode& q = c.qnodes[ref];
    for (int i = 0; i < 4; i++) {
      if (q.ref[i] == Q_EMPTY) continue;
      float l[3], h[3];
      rw(q.ref[i], l, h);
      for (int a = 0; a < 3; a++) { q.lo[a][i] = l[a]; q.hi[a][i] = h[a]; }
    }
    wnode_box(q, lo, hi);
  };
  float lo[3], hi[3];
  if (!ref_is_leaf(c.root)) rb(c.root, lo, hi);
  if (c.qbuilt && !ref_is_leaf(c.qroot)) rw(c.qroot, lo, hi);
}

// Validation of one updated triangle's 18 floats: finite, positions below 2^30 in magnitude
SCN_HD inline bool vertex_data_ok(const float* p1, const float* p2, const float* p3, const float* n1, const float* n2,
                                  const float* n3) {
  bool ok = true;
  for (int a = 0; a < 3; a++) {
    ok = ok && fabsf(p1[a]) < 0x1p30f && fabsf(p2[a]) < 0x1p30f && fabsf(p3[a]) < 0x1p30f;  // (false for NaN, inf)
    ok = ok && trif::finitef_(n1[a]) && trif::finitef_(n2[a]) && trif::finitef_(n3[a]);
  }
  return ok;
}

// New vertices for `count` triangles of a compiled scene: t = first + i (tri_index NULL) or
// tri_index[i] (first = 0).  p1..n3: float[3 * count].  Recomputes tri, trin.xyz, hrec and trx
// (caps as compiled, extrema only growing), lets the culling bound grow, and refits both trees.
// This is the definition; rt_update_geometry does the same on the device.  Returns RT_OK, or
// RT_ERR_ARG with the reason in err and c untouched.
inline int update_geometry(Compiled& c, const int32_t* tri_index, int first, int count, const float* p1, const float* p2,
                           const float* p3, const float* n1, const float* n2, const float* n3, std::string& err) {
  auto fail = [&](const char* msg) {
    err = msg;
    return (int)RT_ERR_ARG;
  };
  if (count < 0) return fail("negative count");
  if (count == 0) return RT_OK;
  if (!p1 || !p2 || !p3 || !n1 || !n2 || !n3) return fail("missing vertex arrays");
  if (tri_index) {
    if (first != 0) return fail("first must be 0 with an index list");
    std::vector<char> seen((size_t)std::max(c.n_tri, 0), 0);
    for (int i = 0; i < count; i++) {
      const int t = tri_index[i];
      if (t < 0 || t >= c.n_tri) return fail("triangle index out of range");
      if (seen[t]) return fail("duplicate triangle index");
      seen[t] = 1;
    }
  } else if (first < 0 || (int64_t)first + count > c.n_tri) {
    return fail("range outside the triangle list");
  }
  for (int i = 0; i < count; i++)
    if (!vertex_data_ok(p1 + 3 * i, p2 + 3 * i, p3 + 3 * i, n1 + 3 * i, n2 + 3 * i, n3 + 3 * i))
      return fail("a position or normal is not finite, or a position is 2^30 or more");
  CullStats cs{c.cull_R, c.cull_K, c.cull_off};
  for (int i = 0; i < count; i++) {
    const size_t t = (size_t)(tri_index ? tri_index[i] : first + i);
    float* tri = &c.tri[12 * t];
    float* trx = &c.trx[12 * t];
    float scratch[12];
    const bool was_flagged = !trif::within_caps(trif::tri_rows(tri, scratch), c.s_cap, c.sc_cap);
    tri_record(p1 + 3 * i, p2 + 3 * i, p3 + 3 * i, n1 + 3 * i, n2 + 3 * i, n3 + 3 * i, tri, &c.trin[12 * t]);
    hit_record(tri, &c.trin[12 * t], &c.hrec[32 * t]);
    const trif::TriQ q = trif::tri_rows(tri, trx);
    const bool flagged = !trif::within_caps(q, c.s_cap, c.sc_cap);
    if (flagged) {
      trx[4] = trx[5] = trx[6] = trx[8] = trx[9] = trx[10] = 0.0f;
    } else {
      c.s_max = std::max(c.s_max, q.S);
      c.sc_max = std::max(c.sc_max, q.sc);
      c.c_min = std::min(c.c_min, q.c);
    }
    c.tri_flagged += (int)flagged - (int)was_flagged;
    cull_merge(cs, cull_tri(p1 + 3 * i, p2 + 3 * i, p3 + 3 * i));
  }
  c.cull_R = cs.R; c.cull_K = cs.K; c.cull_off = cs.off;
  trif::Consts k;
  k.s_max = c.s_max; k.sc_max = c.sc_max; k.c_min = c.c_min;
  trif::form_margin(k);
  c.tri_k1 = k.k1; c.tri_k0 = k.k0;
  refit(c);
  return RT_OK;
}

// The device's refit schedule.  Leaves: {ref, binary parent * 2 + side, 4-wide parent * 4 + slot, 0}
// (-1: the root is the leaf / no 4-wide tree).  Internal nodes of each tree ordered by height (a
// leaf is 0, a node 1 + the highest of its children): nodes of height h are list[off[h - 1] ..
// off[h]), so every child of a node precedes it in an earlier group.
struct RefitPlan {
  std::vector<int32_t> leaves;          // 4 per leaf
  std::vector<int32_t> blist, boff;     // boff[0] = 0, boff.size() = heights + 1
  std::vector<int32_t> qlist, qoff;
};
inline RefitPlan refit_plan(const BNode* nodes, size_t n_nodes, int root, const WNode* qnodes, size_t n_qnodes, int qroot,
                            bool qbuilt, bool has_scene, int n_tri) {
  RefitPlan P;
  P.boff.push_back(0);
  P.qoff.push_back(0);
  if (!has_scene) return P;
  std::vector<int> leaf_at((size_t)std::max(n_tri, 0), -1);  // leaf index by its first triangle
  auto group = [](const std::vector<int>& height, std::vector<int32_t>& list, std::vector<int32_t>& off) {
    int hmax = 0;
    for (int h : height) hmax = std::max(hmax, h);
    off.assign((size_t)hmax + 1, 0);
    for (int h : height) if (h > 0) off[h]++;
    for (int h = 1; h <= hmax; h++) off[h] += off[h - 1];
    list.assign((size_t)off[hmax], 0);
    std::vector<int32_t> at(off.begin(), off.end());
    for (size_t i = 0; i < height.size(); i++)
      if (height[i] > 0) list[at[height[i] - 1]++] = (int32_t)i;
  };
  auto add_leaf = [&](int ref, int bslot) {
    const int f = leaf_first(ref);
    if (f >= 0 && f < n_tri && leaf_at[f] < 0) leaf_at[f] = (int)(P.leaves.size() / 4);
    P.leaves.insert(P.leaves.end(), {ref, bslot, -1, 0});
  };
  if (ref_is_leaf(root)) {
    add_leaf(root, -1);
  } else {
    std::vector<int> height(n_nodes, 0);
    std::function<int(int)> hb = [&](int i) -> int {
      int h = 0;
      for (int k = 0; k < 2; k++) {
        const int r = nodes[i].ref[k];
        if (ref_is_leaf(r)) add_leaf(r, 2 * i + k);
        else h = std::max(h, hb(r));
      }
      return height[i] = h + 1;
    };
    hb(root);
    group(height, P.blist, P.boff);
  }
  if (qbuilt && !ref_is_leaf(qroot)) {
    std::vector<int> height(n_qnodes, 0);
    std::function<int(int)> hq = [&](int i) -> int {
      int h = 0;
      for (int k = 0; k < 4; k++) {
        const int r = qnodes[i].ref[k];
        if (r == Q_EMPTY) continue;
        if (ref_is_leaf(r)) {
          const int f = leaf_first(r);
          if (f >= 0 && f < n_tri && leaf_at[f] >= 0) P.leaves[4 * (size_t)leaf_at[f] + 2] = 4 * i + k;
        } else {
          h = std::max(h, hq(r));
        }
      }
      return height[i] = h + 1;
    };
    hq(qroot);
    group(height, P.qlist, P.qoff);
  }
  return P;
}
inline RefitPlan refit_plan(const Compiled& c) {
  return refit_plan(c.nodes.data(), c.nodes.size(), c.root, c.qnodes.data(), c.qnodes.size(), c.qroot, c.qbuilt,
                    c.has_scene != 0, c.n_tri);
}

// The reference's own AoS encodings (Triangle_encoded: 14 texels, BVHNode_encoded: 4 texels) as an
// rt_scene_soa over arrays this object owns; materials are de-duplicated in first-use order.
struct Decoded {
  std::vector<float> p[6], aa, bb;
  std::vector<int32_t> mid, L, R, N, I;
  std::vector<rt_material> mats;
  rt_scene_soa soa;
};
inline void decode(const float* tri_enc, int32_t n_triangles, const float* node_enc, int32_t n_nodes, Decoded& d) {
  const size_t nt = (size_t)n_triangles;
  for (auto& v : d.p) v.resize(3 * nt);
  d.mid.resize(nt);
  d.mats.clear();
  for (size_t i = 0; i < nt; i++) {
    const float* t = tri_enc + 42 * i;  // Triangle_encoded: 14 texels
    for (int k = 0; k < 6; k++) memcpy(&d.p[k][3 * i], t + 3 * k, 12);
    rt_material m;
    memcpy(&m, t + 18, sizeof(rt_material));
    int found = -1;
    for (size_t q = 0; q < d.mats.size(); q++)
      if (!memcmp(&d.mats[q], &m, sizeof(m))) { found = (int)q; break; }
    if (found < 0) { d.mats.push_back(m); found = (int)d.mats.size() - 1; }
    d.mid[i] = found;
  }
  d.L.resize(n_nodes); d.R.resize(n_nodes); d.N.resize(n_nodes); d.I.resize(n_nodes);
  d.aa.resize(3 * (size_t)n_nodes); d.bb.resize(3 * (size_t)n_nodes);
  for (int i = 0; i < n_nodes; i++) {  // BVHNode_encoded: ints stored as floats (RT:224-230 casts)
    const float* nd = node_enc + 12 * (size_t)i;
    d.L[i] = (int)nd[0]; d.R[i] = (int)nd[1]; d.N[i] = (int)nd[3]; d.I[i] = (int)nd[4];
    memcpy(&d.aa[3 * i], nd + 6, 12);
    memcpy(&d.bb[3 * i], nd + 9, 12);
  }
  rt_scene_soa& s = d.soa;
  s.n_triangles = n_triangles;
  s.p1 = d.p[0].data(); s.p2 = d.p[1].data(); s.p3 = d.p[2].data();
  s.n1 = d.p[3].data(); s.n2 = d.p[4].data(); s.n3 = d.p[5].data();
  s.material_id = d.mid.data();
  s.materials = d.mats.data();
  s.n_materials = (int32_t)d.mats.size();
  s.n_nodes = n_nodes;
  s.node_left = d.L.data(); s.node_right = d.R.data(); s.node_n = d.N.data(); s.node_index = d.I.data();
  s.node_aa = d.aa.data(); s.node_bb = d.bb.data();
}

}  // namespace scn
