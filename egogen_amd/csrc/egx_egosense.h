// What an observation is made of, shared by the env kernels (env.hip) and the observation of the primitive search
// (genop_policy.hip): the walkable polygon of a scene as ring edges, the 32 egosensing rays of one frame (crowd_env_2f.py:524-613)
// against the env's scenes and against the search's polygon with boxes taken out of it, and the unit vector from a canonical
// marker to the target (_get_feature, :680-727).
// Internal linkage, as in the anonymous namespace these came from: each kernel carries its own copy of the same arithmetic.
#pragma once
#include "egx_common.h"

namespace {

constexpr int NRAY = 32;

struct SceneDev {
  const float* edges;   // [E,4]
  const int* edge_off;  // [S+1]
  const float* tris;    // [F,6]
  const int* tri_off;   // [S+1]
  const float* floor_h; // [S]
  const float* map_lin; // [res]
  int map_res;
  // crowd scenes (main_crowd_eval): walkable = square floor minus the world-space marker boxes of the OTHER members
  float* crowd_bbox;    // [G][S][4] (minx,miny,maxx,maxy) or null
  int crowd_G, crowd_S, crowd_k;
  float crowd_half;     // floor is [-half, half]^2 (crowd_env_crowd_eval.py:391)
  int crowd_polygon;    // 1: the exterior is the ring set edges[edge_off[0] .. edge_off[1]) instead of the square floor
                        //    (crowd_env_egobody_eval.py:402 scene_poly = walkable region of the scene's navmesh)
  int crowd_static;     // 1: the other members' boxes are NOT holes (what shapely's Polygon(polygon, holes) evaluates to in
                        //    crowd_env_egobody_eval.py:824)
};

// number of boundary edges of scene `sc_i` and the e-th edge (x0,y0,x1,y1) in float64
__device__ __forceinline__ int scene_num_edges(const SceneDev& sc, int sc_i) {
  if (sc.crowd_bbox)
    return (sc.crowd_polygon ? sc.edge_off[1] - sc.edge_off[0] : 4) + (sc.crowd_static ? 0 : 4 * (sc.crowd_G - 1));
  return sc.edge_off[sc_i + 1] - sc.edge_off[sc_i];
}
__device__ __forceinline__ void scene_edge(const SceneDev& sc, int sc_i, int e, double& x0, double& y0, double& x1, double& y1) {
  if (!sc.crowd_bbox) {
    const float* p = sc.edges + (size_t)(sc.edge_off[sc_i] + e) * 4;
    x0 = p[0]; y0 = p[1]; x1 = p[2]; y1 = p[3];
    return;
  }
  const int n_ext = sc.crowd_polygon ? sc.edge_off[1] - sc.edge_off[0] : 4;
  if (sc.crowd_polygon && e < n_ext) {
    const float* p = sc.edges + (size_t)(sc.edge_off[0] + e) * 4;
    x0 = p[0]; y0 = p[1]; x1 = p[2]; y1 = p[3];
    return;
  }
  float lo[2], hi[2];
  int q;
  if (e < n_ext) {
    lo[0] = lo[1] = -sc.crowd_half; hi[0] = hi[1] = sc.crowd_half;
    q = e;
  } else {
    e -= n_ext - 4;
    int other = (e - 4) >> 2;
    if (other >= sc.crowd_k) ++other;  // skip this member's own box
    const float* b = sc.crowd_bbox + ((size_t)other * sc.crowd_S + sc_i) * 4;
    lo[0] = b[0]; lo[1] = b[1]; hi[0] = b[2]; hi[1] = b[3];
    q = (e - 4) & 3;
  }
  // rectangle corners c0=(lo,lo) c1=(hi,lo) c2=(hi,hi) c3=(lo,hi); edge q = c_q -> c_{q+1}
  const double cx[4] = {lo[0], hi[0], hi[0], lo[0]}, cy[4] = {lo[1], lo[1], hi[1], hi[1]};
  x0 = cx[q]; y0 = cy[q]; x1 = cx[(q + 1) & 3]; y1 = cy[(q + 1) & 3];
}

// ---- the 32 egosensing rays of one frame, float64 like the reference's numpy/shapely path ----------------------------------------
// One core, egosensing_rays, written over an edge source that hands it
//   void for_each_edge(f)                   f(x0, y0, x1, y1) on every boundary edge the rays are tested against, in float64
//   bool contains(ox, oy)                   whether the eye stands on walkable ground; where it does not, every ray reads -1
// The env's source is SceneEdges, the search's is HoleEdges; the core does not know which of them it serves.

// the even-odd test, one edge at a time: the edges a half-line from (ox, oy) towards +x crosses
struct EgoCrossings {
  double ox, oy;
  int crossings;
  __device__ __forceinline__ void operator()(double x0, double y0, double x1, double y1) {
    if ((y0 > oy) != (y1 > oy)) {
      const double xint = x0 + (oy - y0) * (x1 - x0) / (y1 - y0);
      crossings += ox < xint ? 1 : 0;   // an add-with-carry as when the count was a local; `if (...) ++crossings` on a member is a branch
    }
  }
  __device__ __forceinline__ bool odd() const { return (crossings & 1) == 1; }
};

// the ray / edge intersection, one edge at a time: d ends as the nearest hit of the ray from (ox, oy) along (dx, dy), if any is
// nearer than what it started as
struct EgoNearestHit {
  double ox, oy, dx, dy, ray_len, d;
  __device__ __forceinline__ void operator()(double ex0, double ey0, double ex1, double ey1) {
    const double edx = ex1 - ex0, edy = ey1 - ey0;
    const double den = dx * edy - dy * edx;
    if (fabs(den) > 0.0) {
      const double tt = ((ex0 - ox) * edy - (ey0 - oy) * edx) / den;
      const double uu = ((ex0 - ox) * dy - (ey0 - oy) * dx) / den;
      if (tt > 0.0 && tt <= ray_len && uu >= 0.0 && uu <= 1.0 && tt < d) d = tt;
    }
  }
};

// containment + first exit along 32 rays.
// eye/look are computed in float32 first (joint.detach().cpu().numpy() is float32), then promoted.
template <class Edges>
__device__ __forceinline__ void egosensing_rays(const Edges& src, const float* j23, const float* j24, const float* j56,
                                                const float* j57, double ray_len, float* out32 /*[32]*/, int tid, int nthreads) {
  const float lx = j57[0] - j23[0] + j56[0] - j24[0];
  const float ly = j57[1] - j23[1] + j56[1] - j24[1];
  double la0 = (double)lx, la1 = (double)ly;
  const double ln = sqrt(la0 * la0 + la1 * la1);
  la0 /= ln; la1 /= ln;
  const float exf = (j23[0] + j24[0]) / 2.f, eyf = (j23[1] + j24[1]) / 2.f;
  const double ox = (double)exf, oy = (double)eyf;
  // containment (every thread computes it redundantly; E is small)
  const bool inside = src.contains(ox, oy);
  const double PI = 3.14159265358979323846;
  for (int i = tid; i < NRAY; i += nthreads) {
    double d = 0.0;
    if (inside) {
      // np.linspace(-pi/2, pi/2, 32): start + i*step, last sample exactly the stop value
      const double ang = (i == NRAY - 1) ? PI / 2 : -PI / 2 + (double)i * (PI / (double)(NRAY - 1));
      const double ca = cos(ang), sa = sin(ang);
      const double dx = la0 * ca - la1 * sa, dy = la1 * ca + la0 * sa;
      EgoNearestHit hit{ox, oy, dx, dy, ray_len, ray_len};
      src.for_each_edge(hit);
      d = hit.d;
      const double px = ox + dx * d - ox, py = oy + dy * d - oy;  // |end - eye| from the returned coordinates
      d = sqrt(px * px + py * py);
    }
    out32[i] = -1.f + 2.f * (float)(d / ray_len);
  }
}

// The env's source: the edges of scene `scene` through scene_num_edges / scene_edge, containment even-odd over all of them (a
// crowd scene's boxes included: the env's boxes are rings of the polygon like any other).
struct SceneEdges {
  const SceneDev& sc;
  int scene;
  template <class F>
  __device__ __forceinline__ void for_each_edge(F& f) const {
    const int ne = scene_num_edges(sc, scene);
    for (int e = 0; e < ne; ++e) {
      double x0, y0, x1, y1;
      scene_edge(sc, scene, e, x0, y0, x1, y1);
      f(x0, y0, x1, y1);
    }
  }
  __device__ __forceinline__ bool contains(double ox, double oy) const {
    EgoCrossings c{ox, oy, 0};
    for_each_edge(c);
    return c.odd();
  }
};
__device__ void egosensing_frame(const SceneDev& sc, int scene, const float* j23, const float* j24, const float* j56,
                                 const float* j57, double ray_len, float* out32 /*[32]*/, int tid, int nthreads) {
  egosensing_rays(SceneEdges{sc, scene}, j23, j24, j56, j57, ray_len, out32, tid, nthreads);
}

// The search's source (genop_policy.hip): a static polygon MINUS THE UNION of axis-aligned boxes.  The reference's crowd evaluation
// makes the other agents' marker boxes holes of the walkable polygon (dummy_vector_env.py:34-39,81-84, shapely's union_all), so a
// point in two overlapping boxes is in a hole.
//   edges [ne,4] the static ring edges (LDS or global), null with ne = 0: the unbounded plane;  boxes [nb,4] (minx,miny,maxx,maxy)
// The edges are the static ones, then the four of every box (corners and edge order of scene_edge: c0=(lo,lo) c1=(hi,lo)
// c2=(hi,hi) c3=(lo,hi), edge q = c_q -> c_{q+1}).  The eye stands on walkable ground where it lies inside the static polygon
// (even-odd over its edges) and in no box: minx <= x < maxx and miny <= y < maxy, which is what the even-odd test over the four
// edges of ONE box evaluates to.  Even-odd over all the edges would make the overlap of two boxes walkable again.
struct HoleEdges {
  const float* edges;
  int ne;
  const float* boxes;
  int nb;
  template <class F>
  __device__ __forceinline__ void for_each_static_edge(F& f) const {
    for (int e = 0; e < ne; ++e) f(edges[e * 4 + 0], edges[e * 4 + 1], edges[e * 4 + 2], edges[e * 4 + 3]);
  }
  template <class F>
  __device__ __forceinline__ void for_each_edge(F& f) const {
    for_each_static_edge(f);
    for (int k = 0; k < nb; ++k) {
      const double lox = boxes[k * 4 + 0], loy = boxes[k * 4 + 1], hix = boxes[k * 4 + 2], hiy = boxes[k * 4 + 3];
      const double cx[4] = {lox, hix, hix, lox}, cy[4] = {loy, loy, hiy, hiy};
      for (int q = 0; q < 4; ++q) f(cx[q], cy[q], cx[(q + 1) & 3], cy[(q + 1) & 3]);
    }
  }
  __device__ __forceinline__ bool contains(double ox, double oy) const {
    bool inside = true;
    if (edges) {
      EgoCrossings c{ox, oy, 0};
      for_each_static_edge(c);
      inside = c.odd();
    }
    for (int k = 0; k < nb; ++k) {
      const double lox = boxes[k * 4 + 0], loy = boxes[k * 4 + 1], hix = boxes[k * 4 + 2], hiy = boxes[k * 4 + 3];
      if (lox <= ox && ox < hix && loy <= oy && oy < hiy) inside = false;
    }
    return inside;
  }
};

// _get_feature (crowd_env_2f.py:680-727), the part the observation keeps: unit vector from a canonical marker to the target
__device__ __forceinline__ void marker_target_feature(const float* target_l, const float* marker, float* out3) {
  const float fx = target_l[0] - marker[0], fy = target_l[1] - marker[1], fz = target_l[2] - marker[2];
  const float dn = fmaxf(sqrtf(fx * fx + fy * fy + fz * fz), 1e-12f);
  out3[0] = fx / dn; out3[1] = fy / dn; out3[2] = fz / dn;
}
// ... and the clipped 3-D distance pelvis -> target: target_distance (egx_reward.h)

}  // namespace
