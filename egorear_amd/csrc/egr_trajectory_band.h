// The temporal penalty of the clip decoders, written once: egr_trajectory.hip eliminates it with scalar entries,
// egr_raytrack.hip with the same entries times the 3 x 3 identity.
#pragma once

// Row t of lv D1^T D1 + la D2^T D2: the diagonal a, A[t][t+1] = b and A[t][t+2] = c.  Row i of D2 (i = 1..T-2) holds (1, -2, 1) at
// (i-1, i, i+1), so where T < 5 the band is narrower by itself.
__host__ __device__ inline void trj_band(int t, int T, double lv, double la, double& a, double& b, double& c) {
    const int mid = (t >= 1 && t <= T - 2) ? 1 : 0, up = (t + 1 <= T - 2) ? 1 : 0, dn = (t >= 2) ? 1 : 0;
    a = lv * (double)((t > 0 ? 1 : 0) + (t < T - 1 ? 1 : 0)) + la * (double)(up + 4 * mid + dn);
    b = t < T - 1 ? -lv - la * (double)(2 * (mid + up)) : 0.0;
    c = up ? la : 0.0;
}
