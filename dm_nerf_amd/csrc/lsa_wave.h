// lsa_wave.h -- rectangular linear assignment on one wavefront, shared by the object-code loss (criterion.hip) and the
// instance AP evaluation (ins_eval.hip).
//
// Shortest augmenting paths (Crouse 2016), the algorithm scipy.optimize.linear_sum_assignment implements, with its tie rule:
// rows 0..V-1 are assigned to distinct columns of 0..C-1 (V <= C <= LSA_MAXC) at minimum total cost.  Wave 0 runs it; lane j owns
// columns j and j + 64, the column scan is spread over the lanes and the minimum found by a butterfly.  The caller says how a
// cost entry is read: cost(i, j) returns entry (row i, column j) as a double.
#pragma once
#include <hip/hip_runtime.h>

constexpr int LSA_MAXC = 128;

// LDS of the solver: duals u (rows) / v (columns), shortest path costs, the path tree, the matching both ways, visited sets.
struct LsaShared {
    double u[LSA_MAXC], v[LSA_MAXC], spc[LSA_MAXC];
    int path[LSA_MAXC], col4row[LSA_MAXC], row4col[LSA_MAXC];
    unsigned char SR[LSA_MAXC], SC[LSA_MAXC];
};

__device__ __forceinline__ double wave_min_key(double v, int key, int& key_out) {
    // minimum of v over the wave; ties: smaller key.  Returns the minimum, key_out = its key.
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double ov = __shfl_xor(v, off);
        const int ok = __shfl_xor(key, off);
        if (ov < v || (ov == v && ok < key)) { v = ov; key = ok; }
    }
    key_out = key;
    return v;
}

// Called by the 64 lanes of one wave (lane = 0..63).  On return s.col4row[0..V-1] is the column of each row and s.row4col[0..C-1]
// the row of each column (-1: unassigned).
template <class Cost>
__device__ void lsa_solve_wave(LsaShared& s, int V, int C, int lane, Cost cost) {
    for (int j = lane; j < C; j += 64) { s.v[j] = 0.0; s.row4col[j] = -1; }
    for (int i = lane; i < V; i += 64) { s.u[i] = 0.0; s.col4row[i] = -1; }
    __builtin_amdgcn_wave_barrier();
    for (int cur = 0; cur < V; ++cur) {
        for (int j = lane; j < C; j += 64) { s.spc[j] = __builtin_inf(); s.SC[j] = 0; s.path[j] = -1; }
        for (int i = lane; i < V; i += 64) s.SR[i] = 0;
        __builtin_amdgcn_wave_barrier();
        double min_val = 0.0;
        int i = cur, sink = -1;
        while (sink < 0) {
            if (lane == 0) s.SR[i] = 1;
            const double ui = s.u[i];
            double best = __builtin_inf();
            int best_key = 0x7fffffff;
            for (int j = lane; j < C; j += 64) {
                if (s.SC[j]) continue;
                const double r = min_val + cost(i, j) - ui - s.v[j];
                if (r < s.spc[j]) { s.spc[j] = r; s.path[j] = i; }
                const double sj = s.spc[j];
                // ties: an unassigned column first (it ends the search), then the lower index
                const int key = (s.row4col[j] < 0 ? 0 : LSA_MAXC) + j;
                if (sj < best || (sj == best && key < best_key)) { best = sj; best_key = key; }
            }
            int key;
            min_val = wave_min_key(best, best_key, key);
            const int jstar = key >= LSA_MAXC ? key - LSA_MAXC : key;
            if (lane == 0) s.SC[jstar] = 1;
            __builtin_amdgcn_wave_barrier();
            if (s.row4col[jstar] < 0) sink = jstar; else i = s.row4col[jstar];
        }
        // dual updates
        for (int r = lane; r < V; r += 64)
            if (s.SR[r]) s.u[r] += (r == cur) ? min_val : min_val - s.spc[s.col4row[r]];
        for (int j = lane; j < C; j += 64)
            if (s.SC[j]) s.v[j] -= min_val - s.spc[j];
        __builtin_amdgcn_wave_barrier();
        // augment along the path (serial; at most V steps)
        if (lane == 0) {
            int j = sink;
            while (true) {
                const int r = s.path[j];
                s.row4col[j] = r;
                const int prev = s.col4row[r];
                s.col4row[r] = j;
                j = prev;
                if (r == cur) break;
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}
