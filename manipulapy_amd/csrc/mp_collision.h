// Sphere-model collision distances, CHOMP cost and gradients, one row per call (float64, 1..MP_MAX_DOF joints, unrolled).  Header-only
// like mp_kin_vjp.h: the HIP kernel k_collision (mp_kernels.hip) and the CPU twin (mp_cpu.cpp) instantiate the same templates.  The
// conventions and the degenerate cases are stated once, in include/manipula_hip.h (mp_collision_*); this is how they are computed.
//
// Tables (all wave-uniform: the kernel reads them with scalar loads through constant-address-space pointers, the twin through plain ones):
//   MpColSpheres   the robot's spheres SORTED BY LINK, centres in link-local coordinates of the compiled frames (mp_model.h), the
//                  caller's index of each, and first[k] .. first[k + 1] = the run of link k (0 = the fixed base .. n)
//   MpColPair      the self pairs as SORTED indices (the parked centres are addressed by them), in the caller's order
//   MpColWorld     the obstacle count and the point cloud's address (null: none), followed by the obstacles (kind + 16 doubles each)
// The point cloud (mp_cloud.h) is one more obstacle after the O primitives: its header is wave-uniform too, its cells and records are
// per-lane gathers.  Only tables whose CL parameter names the cloud's pointer types carry the query (MpColTables::has_cloud): the
// kernels have an instance with and one without, and a launch on a handle without a cloud runs the code it ran before there were clouds.
//
// Per row: the FK sweep of mp_fk_jac, unrolled over the links.  At link k the Jacobian column of joint k is kept, and every sphere of
// the link's run gets its world centre c = p_k + R_k c_local, is parked (PARK: LDS [sphere][xyz][lane] in the kernel, a local array
// in the twin) and is measured against every obstacle: d = sd_o(c) - r.  The running minimum keeps its witness (n, c, link); the hinge's
// force F = phi'(d) n is summed per sphere and enters the LINK's space-frame wrench W_k = [sum c x F; sum F] - k is a compile-time
// index there.  The pairs follow the sweep: both centres come back from the park, +F goes to a's link and -F to b's through a
// wave-uniform switch over the same compile-time accumulators.  One sweep from the tip then gives grad_j = J_j . sum_{k >= j} W_k, and
// the distance gradients are J_j . [c x n; n] of the witness for j up to its link.
#pragma once

#include "mp_core.h"

constexpr int MP_COL_MAX_SPHERES = 64;
constexpr int MP_COL_SPHERE = 0, MP_COL_CAPSULE = 1, MP_COL_BOX = 2;  // = MP_OBSTACLE_* of the public header
#define MP_COL_TINY 1e-300  // a direction shorter than this is n = 0 (coincident centres, a point on a capsule's axis)

#include "mp_cloud.h"

struct MpColSpheres {
  int S, P;
  int first[MP_MAX_DOF + 2];         // spheres of link k: first[k] <= s < first[k + 1]
  int caller[MP_COL_MAX_SPHERES];    // the caller's index of sorted sphere s
  int link[MP_COL_MAX_SPHERES];
  double radius[MP_COL_MAX_SPHERES];
  double local[MP_COL_MAX_SPHERES][3];
  // motion bounds of the edge check: rho[j - 1][k] = the largest distance a sphere centre of link k can have from the axis of the
  // revolute joint j <= k, whatever the configuration (prismatic joints between them not counted: mp_col_edge_begin adds them per
  // edge); 0 for a prismatic j, for k < j and for a link without spheres
  double rho[MP_MAX_DOF][MP_MAX_DOF + 1];
};
struct MpColPair { int a, b; };
struct MpColObstacle {
  double p[16];  // sphere: c, r;  capsule: p0, p1, r;  box: c, R (row-major, columns = the box axes in the world), half-extents
  int kind, pad;
};
struct MpColWorld {  // the header of the obstacle table; MpColObstacle[O] follows at +16 bytes
  int O, pad;
  const MpColCloud* cloud;  // the point cloud's image (mp_cloud.h), null: none
};
static_assert(sizeof(MpColWorld) == 16, "the obstacles follow at +16 bytes");

// views of the tables: SP / PP / WP / OP are pointers, plain on the host and constant-address-space in the kernel; CL: the pointer
// types of the cloud's image (MpCloudPtrHost, the kernels' own), void for tables that never look for a cloud
template <typename CL> struct MpColHasCloud { static constexpr bool value = true; };
template <> struct MpColHasCloud<void> { static constexpr bool value = false; };
template <typename SP, typename PP, typename WP, typename OP, typename CL = void>
struct MpColTables {
  typedef CL Cloud;
  static constexpr bool has_cloud = MpColHasCloud<CL>::value;
  SP sph;
  PP pairs;
  WP world;
  OP obs;
};
// the cloud of tables that can have one (null: none set); wave-uniform
template <typename TB>
MP_HD const MpColCloud* mp_col_cloud_of(const TB& tb) {
  if constexpr (TB::has_cloud) return tb.world->cloud;
  else return nullptr;
}

// the park of the world centres
struct MpColParkLocal {
  double c[3 * MP_COL_MAX_SPHERES];
  MP_HD void put(int s, double x, double y, double z) { c[3 * s] = x; c[3 * s + 1] = y; c[3 * s + 2] = z; }
  MP_HD void get(int s, double& x, double& y, double& z) const { x = c[3 * s]; y = c[3 * s + 1]; z = c[3 * s + 2]; }
};
struct MpColParkLanes {  // [sphere][xyz][lane]: consecutive lanes hit consecutive 8-byte words
  double* base;          // already offset by the lane
  MP_HD void put(int s, double x, double y, double z) { base[(3 * s) * 64] = x; base[(3 * s + 1) * 64] = y; base[(3 * s + 2) * 64] = z; }
  MP_HD void get(int s, double& x, double& y, double& z) const { x = base[(3 * s) * 64]; y = base[(3 * s + 1) * 64]; z = base[(3 * s + 2) * 64]; }
};

// the running frame of the FK sweep: columns x, y, z of R and the origin p, in the space frame (mp_fk_jac's variables)
struct MpColFrame {
  double x0, x1, x2, y0, y1, y2, z0, z1, z2, p0, p1, p2;
  template <typename MT> MP_HD void base(const MT& M) {
    x0 = M.base_R[0]; x1 = M.base_R[3]; x2 = M.base_R[6];
    y0 = M.base_R[1]; y1 = M.base_R[4]; y2 = M.base_R[7];
    z0 = M.base_R[2]; z1 = M.base_R[5]; z2 = M.base_R[8];
    p0 = M.base_p[0]; p1 = M.base_p[1]; p2 = M.base_p[2];
  }
  template <typename JT> MP_HD void fixed(const JT& J) {  // . Rx(alpha) Tx(a)
    p0 += J.a * x0; p1 += J.a * x1; p2 += J.a * x2;
    const double a0 = y0, a1 = y1, a2 = y2;
    y0 = J.ca * a0 + J.sa * z0; y1 = J.ca * a1 + J.sa * z1; y2 = J.ca * a2 + J.sa * z2;
    z0 = J.ca * z0 - J.sa * a0; z1 = J.ca * z1 - J.sa * a1; z2 = J.ca * z2 - J.sa * a2;
  }
  MP_HD void moved(double c, double s, double d) {  // . Rz(theta) Tz(d)
    const double b0 = x0, b1 = x1, b2 = x2;
    x0 = c * b0 + s * y0; x1 = c * b1 + s * y1; x2 = c * b2 + s * y2;
    y0 = c * y0 - s * b0; y1 = c * y1 - s * b1; y2 = c * y2 - s * b2;
    p0 += d * z0; p1 += d * z1; p2 += d * z2;
  }
};

// the frames of links 1..N at `q` (R row-major, p): the constructor turns home-configuration centres into link-local ones with them
template <int N, typename MT>
MP_HD void mp_col_link_frames(const MT& M, const double (&q)[N], double (&R)[N][9], double (&p)[N][3]) {
  MpJointState<double, N> js;
  mp_joint_state<double, N>(M, q, js);
  MpColFrame f;
  f.base(M);
#pragma unroll
  for (int i = 0; i < N; ++i) {
    if (i > 0) f.fixed(mp_joint_of(M, i));
    f.moved(js.c[i], js.s[i], js.d[i]);
    R[i][0] = f.x0; R[i][1] = f.y0; R[i][2] = f.z0; R[i][3] = f.x1; R[i][4] = f.y1; R[i][5] = f.z1; R[i][6] = f.x2; R[i][7] = f.y2; R[i][8] = f.z2;
    p[i][0] = f.p0; p[i][1] = f.p1; p[i][2] = f.p2;
  }
}

// signed distance of the point (px, py, pz) to one obstacle and its outward unit direction n (0 where it is undefined)
template <typename OB>
MP_HD void mp_col_signed_distance(const OB& ob, double px, double py, double pz, double& sd, double& nx, double& ny, double& nz) {
  const int kind = ob.kind;
  if (kind == MP_COL_BOX) {
    const double dx = px - ob.p[0], dy = py - ob.p[1], dz = pz - ob.p[2];
    // local = R^T (p - c)
    const double l0 = ob.p[3] * dx + ob.p[6] * dy + ob.p[9] * dz;
    const double l1 = ob.p[4] * dx + ob.p[7] * dy + ob.p[10] * dz;
    const double l2 = ob.p[5] * dx + ob.p[8] * dy + ob.p[11] * dz;
    const double s0 = l0 < 0.0 ? -1.0 : 1.0, s1 = l1 < 0.0 ? -1.0 : 1.0, s2 = l2 < 0.0 ? -1.0 : 1.0;  // the sign of an exact zero is +
    const double q0 = mp_abs(l0) - ob.p[12], q1 = mp_abs(l1) - ob.p[13], q2 = mp_abs(l2) - ob.p[14];
    double m0, m1, m2;
    if (q0 > 0.0 || q1 > 0.0 || q2 > 0.0) {  // outside: the distance to the clamped point
      const double e0 = q0 > 0.0 ? q0 : 0.0, e1 = q1 > 0.0 ? q1 : 0.0, e2 = q2 > 0.0 ? q2 : 0.0;
      const double dist = mp_sqrt(e0 * e0 + e1 * e1 + e2 * e2);
      const double inv = dist < MP_COL_TINY ? 0.0 : 1.0 / dist;
      sd = dist;
      m0 = s0 * e0 * inv; m1 = s1 * e1 * inv; m2 = s2 * e2 * inv;
    } else {  // inside (or on the surface): the nearest face, ties to the lowest axis
      const bool f0 = q0 >= q1 && q0 >= q2, f1 = !f0 && q1 >= q2;
      sd = f0 ? q0 : (f1 ? q1 : q2);
      m0 = f0 ? s0 : 0.0; m1 = f1 ? s1 : 0.0; m2 = (!f0 && !f1) ? s2 : 0.0;
    }
    nx = ob.p[3] * m0 + ob.p[4] * m1 + ob.p[5] * m2;
    ny = ob.p[6] * m0 + ob.p[7] * m1 + ob.p[8] * m2;
    nz = ob.p[9] * m0 + ob.p[10] * m1 + ob.p[11] * m2;
    return;
  }
  double cx = ob.p[0], cy = ob.p[1], cz = ob.p[2], r = ob.p[3];
  if (kind == MP_COL_CAPSULE) {
    const double ax = ob.p[3] - cx, ay = ob.p[4] - cy, az = ob.p[5] - cz;
    const double L2 = ax * ax + ay * ay + az * az;
    double t = L2 > 0.0 ? ((px - cx) * ax + (py - cy) * ay + (pz - cz) * az) / L2 : 0.0;  // p0 = p1: a sphere
    t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
    cx += t * ax; cy += t * ay; cz += t * az;
    r = ob.p[6];
  }
  const double dx = px - cx, dy = py - cy, dz = pz - cz;
  const double dist = mp_sqrt(dx * dx + dy * dy + dz * dz);
  const double inv = dist < MP_COL_TINY ? 0.0 : 1.0 / dist;
  sd = dist - r;
  nx = dx * inv; ny = dy * inv; nz = dz * inv;
}

// the CHOMP hinge and its derivative
MP_HD void mp_col_hinge(double d, double eps, double& phi, double& dphi) {
  if (d < 0.0) { phi = 0.5 * eps - d; dphi = -1.0; }
  else if (d < eps) { const double u = d - eps; phi = u * u / (2.0 * eps); dphi = u / eps; }
  else { phi = 0.0; dphi = 0.0; }
}

// The link index as the compiler must take it: a value it cannot relate to the other cases' (it would otherwise fold the chain of
// uniform branches into ONE store at a run-time index, and the accumulators would live in scratch memory instead of registers).
MP_HD int mp_col_uniform(int v) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+s"(v));
#endif
  return v;
}

// W_link += sign [c x F; F], link wave-uniform: a switch over compile-time accumulators (link 0 does not move: nothing kept)
template <int N>
MP_HD void mp_col_wrench_add(double (&W)[6 * N], int link, double sign, double cx, double cy, double cz, double fx, double fy, double fz) {
  const double gx = sign * fx, gy = sign * fy, gz = sign * fz;
  const double mx = cy * gz - cz * gy, my = cz * gx - cx * gz, mz = cx * gy - cy * gx;
#pragma unroll
  for (int k = 0; k < N; ++k)
    if (mp_col_uniform(link) == k + 1) {
      W[6 * k] += mx; W[6 * k + 1] += my; W[6 * k + 2] += mz; W[6 * k + 3] += gx; W[6 * k + 4] += gy; W[6 * k + 5] += gz;
    }
}

template <int N>
struct MpColRow {
  double dist_world, dist_self, cost;
  int arg_world[2], arg_self[2];
  double grad_dist_world[N], grad_dist_self[N], grad[N];  // written only with WANT_GRAD
};

// J_j . [c x n; n]: the derivative along joint j of the distance a point c on a link beyond it moves along n
template <int N>
MP_HD double mp_col_point_dot(const double (&Jc)[6 * N], int j, double cx, double cy, double cz, double nx, double ny, double nz) {
  return Jc[6 * j] * (cy * nz - cz * ny) + Jc[6 * j + 1] * (cz * nx - cx * nz) + Jc[6 * j + 2] * (cx * ny - cy * nx) + Jc[6 * j + 3] * nx +
         Jc[6 * j + 4] * ny + Jc[6 * j + 5] * nz;
}

template <int N, bool WANT_GRAD, typename MT, typename TB, typename PARK>
MP_HD void mp_collision_row(const MT& M, const TB& tb, const double (&q)[N], double eps_world, double eps_self, PARK& park,
                            MpColRow<N>& out) {
  constexpr int G = WANT_GRAD ? 6 * N : 6;
  const double inf = __builtin_huge_val();
  MpJointState<double, N> js;
  mp_joint_state<double, N>(M, q, js);
  const int O = tb.world->O, P = tb.sph->P;
  const MpColCloud* const cloud = mp_col_cloud_of(tb);
  double Jc[G], W[G];  // per joint [w; v] / per link [moment; force]
#pragma unroll
  for (int k = 0; k < G; ++k) { Jc[k] = 0.0; W[k] = 0.0; }
  double cost = 0.0;
  double dw = inf, wnx = 0.0, wny = 0.0, wnz = 0.0, wcx = 0.0, wcy = 0.0, wcz = 0.0;
  int aws = -1, awo = -1, wlink = 0;
  {  // the base's spheres do not move: parked for the pairs, not measured against the world
    const int s1 = tb.sph->first[1];
    for (int s = 0; s < s1; ++s) park.put(s, tb.sph->local[s][0], tb.sph->local[s][1], tb.sph->local[s][2]);
  }
  MpColFrame f;
  f.base(M);
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const auto& J = mp_joint_of(M, i);
    if (i > 0) f.fixed(J);
    if constexpr (WANT_GRAD) {  // the joint axis is fixed in the PARENT link: read before the joint moves the frame (mp_fk_jac)
      const double cx = f.p1 * f.z2 - f.p2 * f.z1, cy = f.p2 * f.z0 - f.p0 * f.z2, cz = f.p0 * f.z1 - f.p1 * f.z0;
      const double r = J.rev, pr = 1.0 - J.rev;
      Jc[6 * i] = r * f.z0; Jc[6 * i + 1] = r * f.z1; Jc[6 * i + 2] = r * f.z2;
      Jc[6 * i + 3] = r * cx + pr * f.z0; Jc[6 * i + 4] = r * cy + pr * f.z1; Jc[6 * i + 5] = r * cz + pr * f.z2;
    }
    f.moved(js.c[i], js.s[i], js.d[i]);
    const int s0 = tb.sph->first[i + 1], s1 = tb.sph->first[i + 2];
    for (int s = s0; s < s1; ++s) {
      const double lx = tb.sph->local[s][0], ly = tb.sph->local[s][1], lz = tb.sph->local[s][2];
      const double cx = f.p0 + f.x0 * lx + f.y0 * ly + f.z0 * lz;
      const double cy = f.p1 + f.x1 * lx + f.y1 * ly + f.z1 * lz;
      const double cz = f.p2 + f.x2 * lx + f.y2 * ly + f.z2 * lz;
      park.put(s, cx, cy, cz);
      const double rs = tb.sph->radius[s];
      const int who = tb.sph->caller[s];
      double fx = 0.0, fy = 0.0, fz = 0.0;
      for (int o = 0; o < O; ++o) {
        double sd, nx, ny, nz;
        mp_col_signed_distance(tb.obs[o], cx, cy, cz, sd, nx, ny, nz);
        const double d = sd - rs;
        if (d < dw) {
          dw = d; aws = who; awo = o;
          if (WANT_GRAD) { wnx = nx; wny = ny; wnz = nz; wcx = cx; wcy = cy; wcz = cz; wlink = i + 1; }
        }
        double phi, dphi;
        mp_col_hinge(d, eps_world, phi, dphi);
        cost += phi;
        if (WANT_GRAD) { fx += dphi * nx; fy += dphi * ny; fz += dphi * nz; }
      }
      if constexpr (TB::has_cloud) {
        if (cloud != nullptr) {  // the cloud: obstacle O + its point's index, O + M where truncated; one hinge term
          double sd, nx, ny, nz;
          int pt;
          mp_cloud_distance<typename TB::Cloud>(cloud, cx, cy, cz, MP_COL_TINY, sd, nx, ny, nz, pt);
          const double d = sd - rs;
          if (d < dw) {
            dw = d; aws = who; awo = O + pt;
            if (WANT_GRAD) { wnx = nx; wny = ny; wnz = nz; wcx = cx; wcy = cy; wcz = cz; wlink = i + 1; }
          }
          double phi, dphi;
          mp_col_hinge(d, eps_world, phi, dphi);
          cost += phi;
          if (WANT_GRAD) { fx += dphi * nx; fy += dphi * ny; fz += dphi * nz; }
        }
      }
      if constexpr (WANT_GRAD) {
        W[6 * i] += cy * fz - cz * fy; W[6 * i + 1] += cz * fx - cx * fz; W[6 * i + 2] += cx * fy - cy * fx;
        W[6 * i + 3] += fx; W[6 * i + 4] += fy; W[6 * i + 5] += fz;
      }
    }
  }
  double ds = inf, snx = 0.0, sny = 0.0, snz = 0.0, sax = 0.0, say = 0.0, saz = 0.0, sbx = 0.0, sby = 0.0, sbz = 0.0;
  int as0 = -1, as1 = -1, slinka = 0, slinkb = 0;
  for (int k = 0; k < P; ++k) {
    const int a = tb.pairs[k].a, b = tb.pairs[k].b;
    double ax, ay, az, bx, by, bz;
    park.get(a, ax, ay, az);
    park.get(b, bx, by, bz);
    const double dx = ax - bx, dy = ay - by, dz = az - bz;
    const double dist = mp_sqrt(dx * dx + dy * dy + dz * dz);
    const double inv = dist < MP_COL_TINY ? 0.0 : 1.0 / dist;
    const double nx = dx * inv, ny = dy * inv, nz = dz * inv;
    const double d = dist - tb.sph->radius[a] - tb.sph->radius[b];
    const int la = tb.sph->link[a], lb = tb.sph->link[b];
    if (d < ds) {
      ds = d; as0 = tb.sph->caller[a]; as1 = tb.sph->caller[b];
      if (WANT_GRAD) { snx = nx; sny = ny; snz = nz; sax = ax; say = ay; saz = az; sbx = bx; sby = by; sbz = bz; slinka = la; slinkb = lb; }
    }
    double phi, dphi;
    mp_col_hinge(d, eps_self, phi, dphi);
    cost += phi;
    if constexpr (WANT_GRAD) {
      const double fx = dphi * nx, fy = dphi * ny, fz = dphi * nz;
      mp_col_wrench_add<N>(W, la, 1.0, ax, ay, az, fx, fy, fz);
      mp_col_wrench_add<N>(W, lb, -1.0, bx, by, bz, fx, fy, fz);
    }
  }
  out.dist_world = dw; out.dist_self = ds; out.cost = cost;
  out.arg_world[0] = aws; out.arg_world[1] = awo; out.arg_self[0] = as0; out.arg_self[1] = as1;
  if constexpr (WANT_GRAD) {
    double A[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // sum_{k >= j} W_k
#pragma unroll
    for (int j = N - 1; j >= 0; --j) {
#pragma unroll
      for (int k = 0; k < 6; ++k) A[k] += W[6 * j + k];
      out.grad[j] = Jc[6 * j] * A[0] + Jc[6 * j + 1] * A[1] + Jc[6 * j + 2] * A[2] + Jc[6 * j + 3] * A[3] + Jc[6 * j + 4] * A[4] +
                    Jc[6 * j + 5] * A[5];
      const double gw = mp_col_point_dot<N>(Jc, j, wcx, wcy, wcz, wnx, wny, wnz);
      out.grad_dist_world[j] = j < wlink ? gw : 0.0;
      const double ga = mp_col_point_dot<N>(Jc, j, sax, say, saz, snx, sny, snz);
      const double gb = mp_col_point_dot<N>(Jc, j, sbx, sby, sbz, snx, sny, snz);
      out.grad_dist_self[j] = (j < slinka ? ga : 0.0) - (j < slinkb ? gb : 0.0);
    }
  }
}

// a non-finite q row: NaN in every float output, -1 in the indices
template <int N, bool WANT_GRAD>
MP_HD void mp_collision_poison(bool bad, MpColRow<N>& out) {
  mp_poison_if(bad, out.dist_world);
  mp_poison_if(bad, out.dist_self);
  mp_poison_if(bad, out.cost);
  out.arg_world[0] = bad ? -1 : out.arg_world[0]; out.arg_world[1] = bad ? -1 : out.arg_world[1];
  out.arg_self[0] = bad ? -1 : out.arg_self[0]; out.arg_self[1] = bad ? -1 : out.arg_self[1];
  if constexpr (WANT_GRAD) {
    mp_poison_if(bad, out.grad_dist_world);
    mp_poison_if(bad, out.grad_dist_self);
    mp_poison_if(bad, out.grad);
  }
}

// the per-row outputs of a call, any of them null
struct MpColOut {
  double* dist_world;
  int* arg_world;  // (rows, 2)
  double* dist_self;
  int* arg_self;   // (rows, 2)
  double *grad_dist_world, *grad_dist_self, *cost, *grad;
};

// One row r of the C entry over plain host rows, for the CPU twin.  (k_collision stores for itself: its n-wide outputs leave through
// the wave-cooperative stores.)
template <int N, bool WANT_GRAD, typename MT, typename TB>
void mp_collision_cpu_row(const MT& M, const TB& tb, const double* q, double eps_world, double eps_self, long r, const MpColOut& O) {
  double a[N];
  for (int j = 0; j < N; ++j) a[j] = q[r * N + j];
  MpBad<double> bad;
  bad.add(a);
  MpColParkLocal park;
  MpColRow<N> o;
  mp_collision_row<N, WANT_GRAD>(M, tb, a, eps_world, eps_self, park, o);
  mp_collision_poison<N, WANT_GRAD>(bad.any(), o);
  if (O.dist_world) O.dist_world[r] = o.dist_world;
  if (O.dist_self) O.dist_self[r] = o.dist_self;
  if (O.cost) O.cost[r] = o.cost;
  if (O.arg_world) { O.arg_world[2 * r] = o.arg_world[0]; O.arg_world[2 * r + 1] = o.arg_world[1]; }
  if (O.arg_self) { O.arg_self[2 * r] = o.arg_self[0]; O.arg_self[2 * r + 1] = o.arg_self[1]; }
  if constexpr (WANT_GRAD) {
    for (int j = 0; j < N; ++j) {
      if (O.grad_dist_world) O.grad_dist_world[r * N + j] = o.grad_dist_world[j];
      if (O.grad_dist_self) O.grad_dist_self[r * N + j] = o.grad_dist_self[j];
      if (O.grad) O.grad[r * N + j] = o.grad[j];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Continuous collision checking of joint-space edges by conservative advancement (the contract: include/manipula_hip.h,
// mp_collision_edges_*).  The kernel k_collision_edges (mp_kernels.hip) and the CPU twin instantiate the same templates.
//
// Per edge, once (mp_col_edge_begin): the n (n + 1) / 2 speed bounds L[ka][kb], 0 <= ka < kb <= n, from the handle's rho table and the
// edge's own prismatic travel.  They are per lane but read at wave-uniform link numbers, so they live in a table of their own beside
// the park (BOUNDS: LDS [entry][lane] in the kernel, a local array in the twin) and never in indexed registers.
// Per configuration (mp_collision_edge_eval): the FK sweep, the park and the candidate loops of mp_collision_row without cost or
// gradients.  Every world candidate of one link shares L[0][link], and c -> c / L is monotone, so the link's smallest distance gives its
// step with one division; a pair's step is compared as c < tau L and divided only where it lowers tau.
constexpr int MP_COL_EDGE_FREE = 0, MP_COL_EDGE_BLOCKED = 1, MP_COL_EDGE_UNDECIDED = 2, MP_COL_EDGE_INVALID = -1;  // = MP_EDGE_*
constexpr int MP_COL_EDGE_MAX_STEPS = 65536;

MP_HD constexpr int mp_col_bound_index(int ka, int kb) { return kb * (kb - 1) / 2 + ka; }  // ka < kb
template <int N>
struct MpColBoundsLocal {
  double v[N * (N + 1) / 2];
  MP_HD void put(int i, double x) { v[i] = x; }
  MP_HD double get(int i) const { return v[i]; }
};
struct MpColBoundsLanes {  // [entry][lane]
  double* base;            // already offset by the lane
  MP_HD void put(int i, double x) { base[i * 64] = x; }
  MP_HD double get(int i) const { return base[i * 64]; }
};
// The dynamic LDS of the one-wave work-queue kernels built on the edge check (k_collision_edges, k_rrt_connect, k_path_shortcut): the
// park of S centres [sphere][xyz][lane], then the speed bounds [entry][lane] at mp_col_queue_bounds_offset doubles.
MP_HD constexpr int mp_col_queue_bounds_offset(int S) { return 3 * 64 * S; }
MP_HD constexpr unsigned mp_col_queue_lds_bytes(int n, int S) {
  return (unsigned)(mp_col_queue_bounds_offset(S) + 64 * (n * (n + 1) / 2)) * (unsigned)sizeof(double);
}
// The wave-wide steps of a state machine (mp_rrt.h, mp_shortcut.h) where one problem runs at a time, as in the CPU twins: the identity.
// The kernels' version over the 64 lanes is MpWaveOpsLanes (mp_kernels.hip).
struct MpWaveOpsSerial {
  MP_HD int wave_max(int v) const { return v; }
  MP_HD bool wave_any(bool b) const { return b; }
};

struct MpColEdgeParams {
  double margin, tol;
  int max_steps, pad;
};
// the per-edge outputs of a call, any of them null
struct MpColEdgeOut {
  int* status;
  double* t;
  int* steps;
  double* clearance;
  int* witness;  // (edges, 3)
};

struct MpColEdgeEval {
  double dist_world, dist_self, tau;  // tau = min (d - margin) / L over the candidates with L > 0, +inf if there is none
  int arg_world[2], arg_self[2];
};

template <int N, typename MT, typename TB, typename PARK, typename BOUNDS>
MP_HD void mp_collision_edge_eval(const MT& M, const TB& tb, const double (&q)[N], double margin, PARK& park, const BOUNDS& L,
                                  MpColEdgeEval& out) {
  const double inf = __builtin_huge_val();
  MpJointState<double, N> js;
  mp_joint_state<double, N>(M, q, js);
  const int O = tb.world->O, P = tb.sph->P;
  const MpColCloud* const cloud = mp_col_cloud_of(tb);
  double dw = inf, tau = inf;
  int aws = -1, awo = -1;
  {
    const int s1 = tb.sph->first[1];
    for (int s = 0; s < s1; ++s) park.put(s, tb.sph->local[s][0], tb.sph->local[s][1], tb.sph->local[s][2]);
  }
  MpColFrame f;
  f.base(M);
#pragma unroll
  for (int i = 0; i < N; ++i) {
    if (i > 0) f.fixed(mp_joint_of(M, i));
    f.moved(js.c[i], js.s[i], js.d[i]);
    const int s0 = tb.sph->first[i + 1], s1 = tb.sph->first[i + 2];
    double dl = inf;  // the link's smallest distance
    for (int s = s0; s < s1; ++s) {
      const double lx = tb.sph->local[s][0], ly = tb.sph->local[s][1], lz = tb.sph->local[s][2];
      const double cx = f.p0 + f.x0 * lx + f.y0 * ly + f.z0 * lz;
      const double cy = f.p1 + f.x1 * lx + f.y1 * ly + f.z1 * lz;
      const double cz = f.p2 + f.x2 * lx + f.y2 * ly + f.z2 * lz;
      park.put(s, cx, cy, cz);
      const double rs = tb.sph->radius[s];
      const int who = tb.sph->caller[s];
      for (int o = 0; o < O; ++o) {
        double sd, nx, ny, nz;
        mp_col_signed_distance(tb.obs[o], cx, cy, cz, sd, nx, ny, nz);
        const double d = sd - rs;
        if (d < dw) { dw = d; aws = who; awo = o; }
        dl = d < dl ? d : dl;
      }
      if constexpr (TB::has_cloud) {
        if (cloud != nullptr) {
          double sd, nx, ny, nz;
          int pt;
          mp_cloud_distance<typename TB::Cloud>(cloud, cx, cy, cz, MP_COL_TINY, sd, nx, ny, nz, pt);
          const double d = sd - rs;
          if (d < dw) { dw = d; aws = who; awo = O + pt; }
          dl = d < dl ? d : dl;
        }
      }
    }
    if (s1 > s0 && (O > 0 || cloud != nullptr)) {
      const double Lw = L.get(mp_col_bound_index(0, i + 1));
      const double c = dl - margin;
      if (Lw > 0.0 && c < tau * Lw) tau = c / Lw;
    }
  }
  double ds = inf;
  int as0 = -1, as1 = -1;
  for (int k = 0; k < P; ++k) {
    const int a = tb.pairs[k].a, b = tb.pairs[k].b;
    double ax, ay, az, bx, by, bz;
    park.get(a, ax, ay, az);
    park.get(b, bx, by, bz);
    const double dx = ax - bx, dy = ay - by, dz = az - bz;
    const double d = mp_sqrt(dx * dx + dy * dy + dz * dz) - tb.sph->radius[a] - tb.sph->radius[b];
    if (d < ds) { ds = d; as0 = tb.sph->caller[a]; as1 = tb.sph->caller[b]; }
    const int la = tb.sph->link[a], lb = tb.sph->link[b];
    if (la != lb) {  // wave-uniform; a pair on one link keeps its distance
      const double Lp = L.get(la < lb ? mp_col_bound_index(la, lb) : mp_col_bound_index(lb, la));
      const double c = d - margin;
      if (Lp > 0.0 && c < tau * Lp) tau = c / Lp;
    }
  }
  out.dist_world = dw; out.dist_self = ds; out.tau = tau;
  out.arg_world[0] = aws; out.arg_world[1] = awo; out.arg_self[0] = as0; out.arg_self[1] = as1;
}

template <int N>
struct MpColEdgeState {
  double qa[N], dq[N];
  double t, clearance;
  int steps, witness[3];
  bool bad;  // a non-finite end point: the edge runs as q = 0 (one step) and is reported INVALID
};

// qa, qb -> the state at t = 0 and the edge's speed bounds.  For link kb the joints are walked from kb down: w_j = rho[j][kb] + the
// prismatic travel passed so far (revolute), 1 (prismatic); L[j - 1][kb] is the running sum of |dq_j| w_j.
template <int N, typename MT, typename SP, typename BOUNDS>
MP_HD void mp_col_edge_begin(const MT& M, const SP& sph, const double (&qa)[N], const double (&qb)[N], MpColEdgeState<N>& S, BOUNDS& L) {
  MpBad<double> bad;
  bad.add(qa);
  bad.add(qb);
  S.bad = bad.any();
  double reach[N];  // max(|qa_j|, |qb_j|)
#pragma unroll
  for (int j = 0; j < N; ++j) {
    S.qa[j] = S.bad ? 0.0 : qa[j];
    S.dq[j] = S.bad ? 0.0 : qb[j] - qa[j];
    reach[j] = S.bad ? 0.0 : mp_max(mp_abs(qa[j]), mp_abs(qb[j]));
  }
#pragma unroll
  for (int kb = 1; kb <= N; ++kb) {
    double e = 0.0, acc = 0.0;
#pragma unroll
    for (int j = kb; j >= 1; --j) {
      const bool rev = mp_joint_of(M, j - 1).rev != 0.0;
      const double w = rev ? sph->rho[j - 1][kb] + e : 1.0;
      acc += mp_abs(S.dq[j - 1]) * w;
      L.put(mp_col_bound_index(j - 1, kb), acc);
      if (!rev) e += reach[j - 1];
    }
  }
  S.t = 0.0;
  S.clearance = __builtin_huge_val();
  S.steps = 0;
  S.witness[0] = -1; S.witness[1] = -1; S.witness[2] = -1;
}

// One evaluation at S.t.  Returns 0 while the edge is running, otherwise 1 + its status (FREE / BLOCKED / UNDECIDED; S.t is then the
// reported t).  An INVALID edge is the caller's to report (S.bad).
template <int N, typename MT, typename TB, typename PARK, typename BOUNDS>
MP_HD int mp_col_edge_iterate(const MT& M, const TB& tb, const MpColEdgeParams& P, MpColEdgeState<N>& S, PARK& park, const BOUNDS& L) {
  double q[N];
#pragma unroll
  for (int j = 0; j < N; ++j) q[j] = S.qa[j] + S.t * S.dq[j];
  MpColEdgeEval ev;
  mp_collision_edge_eval<N>(M, tb, q, P.margin, park, L, ev);
  S.steps += 1;
  const bool world = ev.dist_world <= ev.dist_self;  // equal: world first
  const double d = world ? ev.dist_world : ev.dist_self;
  if (d < S.clearance) {  // of equal minima the first evaluated stays
    S.clearance = d;
    S.witness[0] = world ? 0 : 1;
    S.witness[1] = world ? ev.arg_world[0] : ev.arg_self[0];
    S.witness[2] = world ? ev.arg_world[1] : ev.arg_self[1];
  }
  if (d - P.margin <= P.tol) return 1 + MP_COL_EDGE_BLOCKED;
  if (S.t + ev.tau >= 1.0) { S.t = 1.0; return 1 + MP_COL_EDGE_FREE; }
  if (S.steps >= P.max_steps) return 1 + MP_COL_EDGE_UNDECIDED;
  S.t += ev.tau;
  return 0;
}

// The row a finished edge reports, stored by the kernel and the twin alike (`done`: what mp_col_edge_iterate returned): INVALID
// overrides whatever the zero edge gave.
template <int N>
MP_HD void mp_col_edge_store(const MpColEdgeOut& O, long row, const MpColEdgeState<N>& S, int done) {
  double t = S.t, clearance = S.clearance;
  mp_poison_if(S.bad, t);
  mp_poison_if(S.bad, clearance);
  if (O.status) O.status[row] = S.bad ? MP_COL_EDGE_INVALID : done - 1;
  if (O.t) O.t[row] = t;
  if (O.steps) O.steps[row] = S.bad ? 0 : S.steps;
  if (O.clearance) O.clearance[row] = clearance;
  if (O.witness) {
#pragma unroll
    for (int k = 0; k < 3; ++k) O.witness[3 * row + k] = S.bad ? -1 : S.witness[k];
  }
}

// One edge of the C entry over plain host rows, for the CPU twin.
template <int N, typename MT, typename TB>
void mp_collision_edge_cpu(const MT& M, const TB& tb, const double* q_from, const double* q_to, const MpColEdgeParams& P, long e,
                           const MpColEdgeOut& O) {
  double a[N], b[N];
  for (int j = 0; j < N; ++j) { a[j] = q_from[e * N + j]; b[j] = q_to[e * N + j]; }
  MpColParkLocal park;
  MpColBoundsLocal<N> L;
  MpColEdgeState<N> S;
  mp_col_edge_begin<N>(M, tb.sph, a, b, S, L);
  int done;
  while (!(done = mp_col_edge_iterate<N>(M, tb, P, S, park, L))) {}
  mp_col_edge_store<N>(O, e, S, done);
}
