// Bone-length-constrained skeleton fit over the fisheye rays, and the two small launches that belong with it.
// Per frame, over the active joints p_j (cm, device frame) of a tree of J <= 16 joints:
//   E(p) = sum_j sum_v w_vj dist^2(p_j, ray_vj) + lambda sum_{bones used} (|p_j - p_parent(j)| - L_j)^2 + rho sum_j |p_j - init_j|^2.
// The data term is the triangulation's - rays::make_ray / add_ray of egr_rays.h - and an exact quadratic: half its gradient is
// A_j p_j - b_j.  Levenberg-Marquardt on the Gauss-Newton model: a bone contributes lambda u u^T blocks, u = d / |d|, so every step
// is a block system on the tree,  (H + mu diag H) delta = -g,  eliminated leaf to root in 3 x 3 steps (rays::factor / ldl_solve)
// without fill-in: a child's coupling -lambda u u^T has rank one, so what it hands its parent is one direction and three numbers.
//
// One wave per frame.  Lane v * 16 + j builds the ray of view v of joint j once - the trigonometry - and keeps it; lane j owns joint
// j's block.  Joints of one tree depth eliminate side by side; a parent folds its children in index order (wave-uniform loop, lane
// reads); the back-substitution and the energies exchange points by wave shuffles.  fp64 arithmetic on fp32 operands, no atomics,
// no LDS: a frame's bits depend on its own operands only.
#include "egr_rays.h"

namespace {

constexpr int SK_MAX_J = 16;
// the damping schedule (include/egorear_hip.h states it; tests/skeleton_statement.py follows it)
constexpr double SK_MU0 = 1e-3, SK_MU_DOWN = 0.1, SK_MU_UP = 10.0, SK_MU_MIN = 1e-12, SK_MU_MAX = 1e12;
constexpr double SK_MIN_BONE = 1e-9;     // cm: a shorter bone has no direction

// lane `src` of the wave, src wave-uniform: a register read, not a trip through the LDS crossbar
__device__ inline double sk_read(double x, int src) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), src), hi = __builtin_amdgcn_readlane(__double2hiint(x), src);
    return __hiloint2double(hi, lo);
}

// the same bits in every lane: each level adds the two halves' partial sums, which commutes
__device__ inline double sk_wave_sum(double x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

__device__ inline double sk_wave_max(double x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = fmax(x, __shfl_xor(x, o, 64));
    return x;
}

// a parent table as one kernel argument: 4 bits a joint
__host__ __device__ inline int sk_parent(uint64_t packed, int j) { return (int)((packed >> (4 * j)) & 15u); }

inline bool sk_pack_parents(const int32_t* parents, int32_t J, uint64_t* packed) {
    if (J < 1 || J > SK_MAX_J || parents[0] != 0) return false;
    uint64_t p = 0;
    for (int j = 1; j < J; ++j) {
        if (parents[j] < 0 || parents[j] >= j) return false;
        p |= (uint64_t)parents[j] << (4 * j);
    }
    *packed = p;
    return true;
}

struct sk_frame {            // what a lane keeps for the whole fit
    // its ray (lane v * 16 + j)
    double w, d[3], R[9], t[3];
    // its joint (lane j < J)
    rays::normal_eq A;       // A p = b of the joint's rays
    double q0[3], L;
    int par, depth, maxdepth, V, j;
    bool active, bone_on;
    double lambda, rho;
};

// E at the points `p` (owner lanes), the same bits in every lane; `acc` = the joint's sum_v w dist^2
__device__ inline double sk_energy(const sk_frame& s, const double* p, double& acc) {
    double pj[3], pp[3];
    for (int k = 0; k < 3; ++k) {
        pj[k] = __shfl(p[k], s.j, 64);
        pp[k] = __shfl(p[k], s.par, 64);
    }
    double term = 0.0;
    if (s.w != 0.0) {
        double q[3];
        rays::apply(s.R, s.t, pj, q);
        const double dq = s.d[0] * q[0] + s.d[1] * q[1] + s.d[2] * q[2];
        const double r0 = q[0] - s.d[0] * dq, r1 = q[1] - s.d[1] * dq, r2 = q[2] - s.d[2] * dq;
        term = s.w * (r0 * r0 + r1 * r1 + r2 * r2);
    }
    acc = 0.0;
    for (int v = 0; v < s.V; ++v) acc += __shfl(term, v * 16 + s.j, 64);
    double e = 0.0;
    if (s.active) {
        const double i0 = p[0] - s.q0[0], i1 = p[1] - s.q0[1], i2 = p[2] - s.q0[2];
        e = acc + s.rho * (i0 * i0 + i1 * i1 + i2 * i2);
        if (s.bone_on) {
            const double d0 = p[0] - pp[0], d1 = p[1] - pp[1], d2 = p[2] - pp[2];
            const double r = sqrt(d0 * d0 + d1 * d1 + d2 * d2) - s.L;
            e += s.lambda * r * r;
        }
    }
    return sk_wave_sum(e);
}

// E(p + delta) - E(p), the same bits in every lane, evaluated as a difference - not as the difference of two sums, whose rounding
// (1e-16 E) would decide every step shorter than sqrt(1e-16 E / stiffness), 1e-7 cm along the rays.  The rays and the prior are
// quadratic: 2 gq . delta + delta^T (A + rho I) delta, exactly.  A bone: lambda (len' - len)(r + r'), len' - len = (dd . (d + d')) /
// (len + len') with dd = delta_j - delta_parent.
__device__ inline double sk_energy_change(const sk_frame& s, const double* p, const double* delta, const double* gq) {
    double pp[3], dpar[3];
    for (int k = 0; k < 3; ++k) {
        pp[k] = __shfl(p[k], s.par, 64);
        dpar[k] = __shfl(delta[k], s.par, 64);
    }
    double e = 0.0;
    if (s.active) {
        const rays::normal_eq& A = s.A;
        const double a0 = (A.a00 + s.rho) * delta[0] + A.a01 * delta[1] + A.a02 * delta[2];
        const double a1 = A.a01 * delta[0] + (A.a11 + s.rho) * delta[1] + A.a12 * delta[2];
        const double a2 = A.a02 * delta[0] + A.a12 * delta[1] + (A.a22 + s.rho) * delta[2];
        e = (2.0 * gq[0] + a0) * delta[0] + (2.0 * gq[1] + a1) * delta[1] + (2.0 * gq[2] + a2) * delta[2];
        if (s.bone_on) {
            const double d0 = p[0] - pp[0], d1 = p[1] - pp[1], d2 = p[2] - pp[2];
            const double dd0 = delta[0] - dpar[0], dd1 = delta[1] - dpar[1], dd2 = delta[2] - dpar[2];
            const double n0 = d0 + dd0, n1 = d1 + dd1, n2 = d2 + dd2;
            const double len = sqrt(d0 * d0 + d1 * d1 + d2 * d2), len2 = sqrt(n0 * n0 + n1 * n1 + n2 * n2);
            const double sum = len + len2;
            const double dlen = sum > 0.0 ? (dd0 * (d0 + n0) + dd1 * (d1 + n1) + dd2 * (d2 + n2)) / sum : 0.0;
            e += s.lambda * dlen * ((len - s.L) + (len2 - s.L));
        }
    }
    return sk_wave_sum(e);
}

// One damped Gauss-Newton system at `p`: delta (owner lanes), g = dE/dp / 2 of the lane's joint and gq, the part of g that the
// quadratic terms - rays and prior - contribute.  false: a block did not factor.  Without `want_step` only g is made: the children
// are folded, nothing is factored, delta is 0.
// One block that does not factor refuses the step for the whole frame, not for its tree alone: E is the frame's.  mu diag H is what
// makes a rank-2 block definite (lambda = 0, a joint kept by one ray and its bone); were an entry of that diagonal exactly 0 - a ray
// along a coordinate axis of the device frame - every step of that frame would be refused and its joints stay at their init.
template <bool want_step>
__device__ inline bool sk_solve(const sk_frame& s, const double* p, double mu, int J, double* delta, double* g, double* gq) {
    const int lane = threadIdx.x;
    const double lambda = s.lambda;
    double pp[3];
    for (int k = 0; k < 3; ++k) pp[k] = __shfl(p[k], s.par, 64);
    double u[3] = {0.0, 0.0, 0.0}, lr = 0.0;
    if (s.bone_on) {
        const double d0 = p[0] - pp[0], d1 = p[1] - pp[1], d2 = p[2] - pp[2];
        const double len = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
        if (len >= SK_MIN_BONE) {
            const double inv = 1.0 / len;
            u[0] = d0 * inv;
            u[1] = d1 * inv;
            u[2] = d2 * inv;
        }
        lr = lambda * (len - s.L);
    }
    double h00 = 0, h01 = 0, h02 = 0, h11 = 0, h12 = 0, h22 = 0;      // the joint's block of H / 2
    g[0] = g[1] = g[2] = gq[0] = gq[1] = gq[2] = 0.0;
    if (s.active) {
        const rays::normal_eq& A = s.A;
        gq[0] = A.a00 * p[0] + A.a01 * p[1] + A.a02 * p[2] - A.rhs[0] + s.rho * (p[0] - s.q0[0]);
        gq[1] = A.a01 * p[0] + A.a11 * p[1] + A.a12 * p[2] - A.rhs[1] + s.rho * (p[1] - s.q0[1]);
        gq[2] = A.a02 * p[0] + A.a12 * p[1] + A.a22 * p[2] - A.rhs[2] + s.rho * (p[2] - s.q0[2]);
        for (int k = 0; k < 3; ++k) g[k] = gq[k] + lr * u[k];
        h00 = A.a00 + s.rho + lambda * u[0] * u[0];
        h01 = A.a01 + lambda * u[0] * u[1];
        h02 = A.a02 + lambda * u[0] * u[2];
        h11 = A.a11 + s.rho + lambda * u[1] * u[1];
        h12 = A.a12 + lambda * u[1] * u[2];
        h22 = A.a22 + s.rho + lambda * u[2] * u[2];
    }
    double c00 = 0, c01 = 0, c02 = 0, c11 = 0, c12 = 0, c22 = 0, radd[3] = {0, 0, 0};     // what the eliminated children take / add
    double y[3] = {0, 0, 0}, z[3] = {0, 0, 0}, m_a = 0.0, m_t = 0.0;
    bool fail = false;
    for (int level = s.maxdepth; level >= 0; --level) {
        for (int c = 1; c < J; ++c) {                    // wave-uniform: the children of this level's joints, in index order
            if (__builtin_amdgcn_readlane(s.depth, c) != level + 1) continue;
            const int pc = __builtin_amdgcn_readlane(s.par, c);
            const double u0 = sk_read(u[0], c), u1 = sk_read(u[1], c), u2 = sk_read(u[2], c);
            const double clr = sk_read(lr, c), ca = sk_read(m_a, c), ct = sk_read(m_t, c);
            if (lane == pc) {
                g[0] -= clr * u0;
                g[1] -= clr * u1;
                g[2] -= clr * u2;
                h00 += lambda * u0 * u0;
                h01 += lambda * u0 * u1;
                h02 += lambda * u0 * u2;
                h11 += lambda * u1 * u1;
                h12 += lambda * u1 * u2;
                h22 += lambda * u2 * u2;
                c00 += ca * u0 * u0;
                c01 += ca * u0 * u1;
                c02 += ca * u0 * u2;
                c11 += ca * u1 * u1;
                c12 += ca * u1 * u2;
                c22 += ca * u2 * u2;
                radd[0] += ct * u0;
                radd[1] += ct * u1;
                radd[2] += ct * u2;
            }
        }
        if (want_step && s.active && s.depth == level) {
            rays::normal_eq S;
            S.a00 = h00 + mu * h00 - c00;
            S.a01 = h01 - c01;
            S.a02 = h02 - c02;
            S.a11 = h11 + mu * h11 - c11;
            S.a12 = h12 - c12;
            S.a22 = h22 + mu * h22 - c22;
            for (int k = 0; k < 3; ++k) S.rhs[k] = radd[k] - g[k];
            rays::ldl f;
            if (!rays::factor(S, 0.0, f)) {
                fail = true;
            } else {
                rays::ldl_solve(f, S.rhs, y);
                if (s.bone_on) {     // delta = y + lambda (u . delta_parent) z: what the parent needs of it is  u . z  and  u . y
                    rays::ldl_solve(f, u, z);
                    m_a = lambda * lambda * (u[0] * z[0] + u[1] * z[1] + u[2] * z[2]);
                    m_t = lambda * (u[0] * y[0] + u[1] * y[1] + u[2] * y[2]);
                }
            }
        }
    }
    for (int k = 0; k < 3; ++k) delta[k] = y[k];
    for (int level = 1; level <= s.maxdepth; ++level) {
        double dp[3];
        for (int k = 0; k < 3; ++k) dp[k] = __shfl(delta[k], s.par, 64);
        if (s.active && s.depth == level) {
            const double a = lambda * (u[0] * dp[0] + u[1] * dp[1] + u[2] * dp[2]);
            for (int k = 0; k < 3; ++k) delta[k] = y[k] + a * z[k];
        }
    }
    return !__any(fail);
}

__global__ __launch_bounds__(64) void skeleton_fit_kernel(const float* coords, const float* conf, const float* cams, const float* ctm,
                                                          uint64_t parents, const float* bone_length, int per_frame, const float* init,
                                                          const uint8_t* init_ok, int V, int J, float sx, float sy, float thr,
                                                          float min_det_ratio, float lambda, float rho, int iterations, float* pose,
                                                          float* ray_cost, float* bone, uint8_t* valid, float* energy0, float* energy,
                                                          float* grad, int32_t* steps) {
    const int b = blockIdx.x, lane = threadIdx.x;
    sk_frame s;
    s.j = lane & 15;
    s.V = V;
    s.lambda = (double)lambda;
    s.rho = (double)rho;
    const int v = lane >> 4;
    rays::normal_eq n;
    s.w = 0.0;
    for (int k = 0; k < 3; ++k) s.d[k] = s.t[k] = 0.0;
    for (int k = 0; k < 9; ++k) s.R[k] = 0.0;
    if (s.j < J && v < V) {
        rays::ray ry;
        rays::make_ray(coords, conf, cams + v * rays::REC, ((int64_t)b * V + v) * J + s.j, (double)sx, (double)sy, thr, ry);
        rays::extrinsics(cams + v * rays::REC, ctm, (int64_t)b * V + v, s.R, s.t);
        s.w = ry.w;
        for (int k = 0; k < 3; ++k) s.d[k] = ry.d[k];
        if (ry.w != 0.0) rays::add_ray(s.R, s.t, ry.d, ry.w, n);
    }
    // the views of a joint meet in its lane, in view order
    double wsum = 0.0;
    int used = 0;
    for (int vv = 0; vv < V; ++vv) {
        const int src = vv * 16 + s.j;
        s.A.a00 += __shfl(n.a00, src, 64);
        s.A.a01 += __shfl(n.a01, src, 64);
        s.A.a02 += __shfl(n.a02, src, 64);
        s.A.a11 += __shfl(n.a11, src, 64);
        s.A.a12 += __shfl(n.a12, src, 64);
        s.A.a22 += __shfl(n.a22, src, 64);
        for (int k = 0; k < 3; ++k) s.A.rhs[k] += __shfl(n.rhs[k], src, 64);
        const double wv = __shfl(s.w, src, 64);
        wsum += wv;
        used += wv != 0.0 ? 1 : 0;
    }
    const bool own = lane < J;
    rays::ldl f0;
    const bool tri_ok = own && used >= 2 && rays::factor(s.A, (double)min_det_ratio, f0);
    bool init_fine = false, constrained = false;
    s.q0[0] = s.q0[1] = s.q0[2] = s.L = 0.0;
    s.par = 0;
    if (own) {
        const int64_t at = (int64_t)b * J + lane;
        const float i0 = init[at * 3 + 0], i1 = init[at * 3 + 1], i2 = init[at * 3 + 2];
        init_fine = init_ok[at] != 0 && isfinite(i0) && isfinite(i1) && isfinite(i2);
        if (init_fine) {
            s.q0[0] = (double)i0;
            s.q0[1] = (double)i1;
            s.q0[2] = (double)i2;
        }
        s.par = sk_parent(parents, lane);
        const float Lf = bone_length[(per_frame ? (int64_t)b * J : 0) + lane];
        constrained = lane > 0 && Lf > 0.f && isfinite(Lf);
        s.L = constrained ? (double)Lf : 0.0;
    }
    // which joints take part, decided once, in index order (a parent before its children)
    unsigned long long act = 0;
    for (int c = 0; c < J; ++c) {
        const bool a = init_fine && (rho > 0.f || tri_ok || (used >= 1 && constrained && ((act >> s.par) & 1ull)));
        act |= __ballot(lane == c && a);
    }
    s.active = own && ((act >> lane) & 1ull);
    s.bone_on = s.active && constrained && ((act >> s.par) & 1ull);
    s.depth = 0;
    s.maxdepth = 0;
    for (int c = 1; c < J; ++c) {                 // depth in the forest of used bones
        const int dp = __shfl(s.depth, s.par, 64);
        if (lane == c && s.bone_on) s.depth = dp + 1;
        const int dc = __builtin_amdgcn_readlane(s.depth, c);
        s.maxdepth = dc > s.maxdepth ? dc : s.maxdepth;
    }

    double p[3] = {s.q0[0], s.q0[1], s.q0[2]}, acc, g[3], gq[3], delta[3];
    if (!s.active) p[0] = p[1] = p[2] = 0.0;
    const double E0 = sk_energy(s, p, acc);
    double mu = SK_MU0;
    int nsteps = 0;
    for (int it = 0; it < iterations; ++it) {
        const bool solved = sk_solve<true>(s, p, mu, J, delta, g, gq);
        if (!s.active) delta[0] = delta[1] = delta[2] = 0.0;
        const double dE = sk_energy_change(s, p, delta, gq);
        if (solved && dE <= 0.0) {          // (a NaN fails the comparison: such a step is not kept)
            for (int k = 0; k < 3; ++k) p[k] += delta[k];
            ++nsteps;
            mu = fmax(mu * SK_MU_DOWN, SK_MU_MIN);
        } else {
            mu = fmin(mu * SK_MU_UP, SK_MU_MAX);
        }
    }
    sk_solve<false>(s, p, mu, J, delta, g, gq);   // the gradient at the result
    const double E = sk_energy(s, p, acc);        // (no kept step raised E; this sum and E0 round on their own)
    double gm = s.active ? 2.0 * fmax(fabs(g[0]), fmax(fabs(g[1]), fabs(g[2]))) : 0.0;
    gm = sk_wave_max(gm);
    double pp[3];
    for (int k = 0; k < 3; ++k) pp[k] = __shfl(p[k], s.par, 64);
    if (own) {
        const int64_t at = (int64_t)b * J + lane;
        for (int k = 0; k < 3; ++k) pose[at * 3 + k] = s.active ? (float)p[k] : 0.f;
        ray_cost[at] = s.active && wsum > 0.0 ? (float)(acc / wsum) : 0.f;
        const double d0 = p[0] - pp[0], d1 = p[1] - pp[1], d2 = p[2] - pp[2];
        bone[at] = s.bone_on ? (float)sqrt(d0 * d0 + d1 * d1 + d2 * d2) : 0.f;
        valid[at] = s.active ? 1 : 0;
    }
    if (lane == 0) {
        energy0[b] = (float)E0;
        energy[b] = (float)E;
        grad[b] = (float)gm;
        steps[b] = act ? nsteps : 0;          // (a frame without an active joint gives zeros)
    }
}

// One thread per bone: fp64 sums over the frames in frame order, two passes (the mean, then the deviations from it).
__global__ __launch_bounds__(64) void bone_lengths_kernel(const float* pose, const uint8_t* valid, uint64_t parents, int B, int J, float* length,
                                                          float* spread, int32_t* count) {
    const int j = threadIdx.x;
    if (j >= J) return;
    const int par = sk_parent(parents, j);
    double sum = 0.0, dev = 0.0;
    int n = 0;
    for (int pass = 0; pass < 2 && j > 0; ++pass) {
        const double mean = pass && n ? sum / n : 0.0;
        for (int b = 0; b < B; ++b) {
            const int64_t a = (int64_t)b * J + j, c = (int64_t)b * J + par;
            if (!valid[a] || !valid[c]) continue;
            const double d0 = (double)pose[a * 3] - (double)pose[c * 3], d1 = (double)pose[a * 3 + 1] - (double)pose[c * 3 + 1],
                         d2 = (double)pose[a * 3 + 2] - (double)pose[c * 3 + 2];
            const double len = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
            if (pass == 0) {
                sum += len;
                ++n;
            } else {
                dev += (len - mean) * (len - mean);
            }
        }
    }
    length[j] = n ? (float)(sum / n) : 0.f;
    spread[j] = n ? (float)sqrt(dev / n) : 0.f;
    count[j] = n;
}

// One thread per frame walks the tree in index order; a moved parent is read back from `out`, which this thread wrote.
__global__ __launch_bounds__(64) void skeleton_resize_kernel(const float* pose, const uint8_t* valid, uint64_t parents, const float* bone_length,
                                                             int per_frame, int B, int J, float* out) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const int64_t base = (int64_t)b * J;
    for (int j = 0; j < J; ++j) {
        const int64_t a = base + j, c = base + sk_parent(parents, j);
        const float x0 = pose[a * 3], x1 = pose[a * 3 + 1], x2 = pose[a * 3 + 2];
        float o0 = x0, o1 = x1, o2 = x2;
        if (j > 0 && valid[a] && valid[c]) {
            double d0 = (double)x0 - (double)pose[c * 3], d1 = (double)x1 - (double)pose[c * 3 + 1], d2 = (double)x2 - (double)pose[c * 3 + 2];
            const double len = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
            const float Lf = bone_length[(per_frame ? base : 0) + j];
            if (Lf > 0.f && isfinite(Lf) && len >= SK_MIN_BONE) {      // else the bone keeps its vector
                const double m = (double)Lf / len;
                d0 *= m;
                d1 *= m;
                d2 *= m;
            }
            o0 = (float)((double)out[c * 3] + d0);
            o1 = (float)((double)out[c * 3 + 1] + d1);
            o2 = (float)((double)out[c * 3 + 2] + d2);
        }
        out[a * 3] = o0;
        out[a * 3 + 1] = o1;
        out[a * 3 + 2] = o2;
    }
}

inline bool sk_weight_ok(float w) { return w >= 0.f && w <= 3.0e38f; }

}  // namespace

extern "C" int egr_skeleton_fit_f32(const float* coords, const float* conf, const float* cams, const float* ctm, const int32_t* parents,
                                    const float* bone_length, int32_t bone_length_per_frame, const float* init, const uint8_t* init_ok,
                                    int32_t B, int32_t V, int32_t J, float sx, float sy, float threshold, float min_det_ratio, float lambda,
                                    float rho, int32_t iterations, float* pose, float* ray_cost, float* bone, uint8_t* valid,
                                    float* energy0, float* energy, float* grad, int32_t* steps, void* stream) {
    if (!coords || !conf || !cams || !parents || !bone_length || !init || !init_ok || !pose || !ray_cost || !bone || !valid || !energy0 ||
        !energy || !grad || !steps)
        return EGR_ENULL;
    uint64_t packed = 0;
    if (!rays::shape_ok(B, V, J, sx, sy, min_det_ratio) || threshold != threshold || !sk_pack_parents(parents, J, &packed) ||
        !sk_weight_ok(lambda) || !sk_weight_ok(rho) || iterations < 1 || iterations > 256)
        return EGR_EINVAL;
    hipLaunchKernelGGL(skeleton_fit_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, coords, conf, cams, ctm, packed, bone_length,
                       bone_length_per_frame ? 1 : 0, init, init_ok, V, J, sx, sy, threshold, min_det_ratio, lambda, rho, iterations, pose,
                       ray_cost, bone, valid, energy0, energy, grad, steps);
    return egr_launch_status();
}

extern "C" int egr_bone_lengths_f32(const float* pose, const uint8_t* valid, const int32_t* parents, int32_t B, int32_t J, float* length,
                                    float* spread, int32_t* count, void* stream) {
    if (!pose || !valid || !parents || !length || !spread || !count) return EGR_ENULL;
    uint64_t packed = 0;
    if (B < 1 || (int64_t)B * J >= (1 << 30) || !sk_pack_parents(parents, J, &packed)) return EGR_EINVAL;
    hipLaunchKernelGGL(bone_lengths_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, pose, valid, packed, B, J, length, spread, count);
    return egr_launch_status();
}

extern "C" int egr_skeleton_resize_f32(const float* pose, const uint8_t* valid, const int32_t* parents, const float* bone_length,
                                       int32_t bone_length_per_frame, int32_t B, int32_t J, float* out, void* stream) {
    if (!pose || !valid || !parents || !bone_length || !out) return EGR_ENULL;
    uint64_t packed = 0;
    if (B < 1 || (int64_t)B * J >= (1 << 30) || pose == out || !sk_pack_parents(parents, J, &packed)) return EGR_EINVAL;
    hipLaunchKernelGGL(skeleton_resize_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, (hipStream_t)stream, pose, valid, packed,
                       bone_length, bone_length_per_frame ? 1 : 0, B, J, out);
    return egr_launch_status();
}
