// surrogate.hip.h — the search controller's LSTM surrogate (mfas_amd/search/surrogate.py: SimpleRecurrentSurrogate.forward_unrolled)
// trained and queried in three kernels (part of the single translation unit mfas_hip.hip):
//   k_surr_grad     one workgroup per 16-row tile of a bucket: the whole forward t = 0..L-1, the loss, the backward through time, and
//                   the tile's PARTIAL gradient of every parameter into its own slot of the partials arena [tile][P];
//   k_surr_adam     one thread per parameter: the tiles' partials summed in tile order (no atomics), scaled by 1/n, torch's Adam
//                   (float32 moments, the update itself rounded once from float64);
//   k_surr_forward  the forward alone, (L, n, n_in) -> (n) predictions, through the same surr_forward_tile as k_surr_grad.
// A train step is the two launches k_surr_grad, k_surr_adam on one stream; nothing waits for another workgroup inside a launch.
//
// The network: e_t = sigmoid(x_t We^T + be); gates = e_t Wih^T + bih + h Whh^T + bhh (i, f, g, o); c = s(f) c + s(i) tanh(g);
// h = s(o) tanh(c); pred = sigmoid(h_L wo^T + bo); loss = mean((pred - y)^2).  Parameters are one flat buffer in state_dict order.
// E and H are padded to multiples of 16 in LDS and in the tile's scratch only (padded e, h, c are exactly 0; the parameter loads of
// padded rows / columns are predicated to 0).  Gate and weight-gradient contractions are f32 MFMAs (16x16x4); a 16-wide k group is
// taken in the order k = 4 * (lane >> 4) + s for MFMA s = 0..3, so that a lane's four A (and B) values are 16 contiguous bytes.
#pragma once

#define SURR_TM 16            // rows per workgroup
#define SURR_THREADS 256      // 4 waves
#define SURR_MAX_IN 8
#define SURR_MAX_ROWS (int64_t(1) << 27)

struct SurrDims {
    int32_t n_in, E, H, Ep, Hp, L, vec, P;      // vec: every weight row is 16-byte aligned (float4 parameter loads)
    int32_t o_be, o_wih, o_whh, o_bih, o_bhh, o_wo, o_bo, _pad;      // flat offsets (We is at 0)
    int64_t n;
};

// LDS map (float offsets).  Forward: xs [L][16][8], es [16][SE], h0 / h1 [16][SH], cs [16][SH], pr [32] (pred, dz).
// Backward adds: dh, dc [16][SH], dgs [16][SG] (the four gates' pre-activation gradients of one step), dps [L][16][SE].
struct SurrLds { int32_t SE, SH, SG, xs, es, h0, h1, cs, pr, dh, dc, dgs, dps, total; };
__host__ __device__ inline SurrLds surr_lds(const int Ep, const int Hp, const int L, const bool grad) {
    SurrLds m;
    m.SE = Ep + 4; m.SH = Hp + 4; m.SG = 4 * Hp + 4;
    int o = 0;
    m.xs = o; o += L * SURR_TM * SURR_MAX_IN;
    m.es = o; o += SURR_TM * m.SE;
    m.h0 = o; o += SURR_TM * m.SH;
    m.h1 = o; o += SURR_TM * m.SH;
    m.cs = o; o += SURR_TM * m.SH;
    m.pr = o; o += 32;
    m.dh = m.dc = m.dgs = m.dps = o;
    if (grad) {
        m.dh = o; o += SURR_TM * m.SH;
        m.dc = o; o += SURR_TM * m.SH;
        m.dgs = o; o += SURR_TM * m.SG;
        m.dps = o; o += L * SURR_TM * m.SE;
    }
    m.total = o;
    return m;
}

// What one step of one tile keeps for the backward pass, in the tile's scratch: the gates i, f, g, o, then c and h ([16][Hp] each), then
// e ([16][Ep]).  The backward pass overwrites the four gate blocks with their pre-activation gradients.
#define SURR_KEEP_C 4
#define SURR_KEEP_H 5
__host__ __device__ inline int64_t surr_keep_floats(const int Ep, const int Hp) { return (int64_t)SURR_TM * (6 * Hp + Ep); }

__device__ __forceinline__ float surr_sigmoid(const float x) { return 1.0f / (1.0f + expf(-x)); }

// four consecutive floats of a parameter row (zeros beyond K or when the row is padding)
__device__ __forceinline__ f32x4 surr_ldrow4(const float* __restrict__ row, const int k, const int K, const bool rowok, const bool vec) {
    f32x4 r = {0.f, 0.f, 0.f, 0.f};
    if (rowok) {
        if (vec) {
            if (k < K) r = *reinterpret_cast<const f32x4*>(row + k);
        } else {
#pragma unroll
            for (int s = 0; s < 4; ++s)
                if (k + s < K) r[s] = row[k + s];
        }
    }
    return r;
}

// acc[q] += A[16 rows][K] * W[(q * H + j) row][K]^T for the 16 hidden units j of column block jb and the four gates q
__device__ __forceinline__ void surr_gate_mac(f32x4 (&acc)[4], const float* a_lds, const int stride, const float* __restrict__ W, const int K,
                                              const int Kp, const int H, const int jb, const int l, const bool vec) {
    const int li = l & 15, lk = l >> 4, jj = jb * 16 + li;
    const bool jok = jj < H;
    for (int k16 = 0; k16 < Kp; k16 += 16) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(a_lds + li * stride + k16 + 4 * lk);
        f32x4 b[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) b[q] = surr_ldrow4(W + (int64_t)(q * H + jj) * K, k16 + 4 * lk, K, jok, vec);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] = MFMA16(a[s], b[q][s], acc[q]);
        }
    }
}

// The forward of rows [row0, row0 + 16) of a bucket.  KEEP: what the backward pass needs goes to `keep` ([L][surr_keep_floats]).
// Leaves the last h in LDS (returned offset), the predictions in lds[m.pr .. m.pr + 16), x in lds[m.xs ..]; ends with a barrier.
template <bool KEEP>
__device__ __forceinline__ int surr_forward_tile(const SurrDims& d, const SurrLds& m, const float* __restrict__ w, const float* __restrict__ x,
                                                 const int64_t row0, float* lds, float* keep) {
    const int tid = (int)threadIdx.x, wv = tid >> 6, l = tid & 63;
    const int E = d.E, H = d.H, Ep = d.Ep, Hp = d.Hp, n_in = d.n_in;
    const bool vec = d.vec != 0;
    const int64_t per_t = surr_keep_floats(Ep, Hp);
    for (int i = tid; i < d.L * SURR_TM * SURR_MAX_IN; i += SURR_THREADS) {
        const int k = i & 7, r = (i >> 3) & 15, t = i >> 7;
        float v = 0.f;
        if (row0 + r < d.n && k < n_in) v = x[((int64_t)t * d.n + row0 + r) * n_in + k];
        lds[m.xs + i] = v;
    }
    for (int i = tid; i < SURR_TM * m.SH; i += SURR_THREADS) { lds[m.h0 + i] = 0.f; lds[m.h1 + i] = 0.f; lds[m.cs + i] = 0.f; }
    __syncthreads();
    int hcur = m.h0, hnext = m.h1;
    for (int t = 0; t < d.L; ++t) {
        float* kt = KEEP ? keep + t * per_t : nullptr;
        // embedding (VALU): e[r][j] = sigmoid(x[r] . We[j] + be[j]); padded columns are 0
        for (int i = tid; i < SURR_TM * Ep; i += SURR_THREADS) {
            const int r = i / Ep, j = i - r * Ep;
            float e = 0.f;
            if (j < E) {
                float s = 0.f;
                for (int k = 0; k < n_in; ++k) s = s + lds[m.xs + (t * SURR_TM + r) * SURR_MAX_IN + k] * w[j * n_in + k];
                e = surr_sigmoid(s + w[d.o_be + j]);
            }
            lds[m.es + r * m.SE + j] = e;
            if (KEEP) kt[6 * SURR_TM * Hp + i] = e;
        }
        __syncthreads();
        // gates (MFMA) and the cell, 16 hidden units x 4 gates per wave and pass
        for (int jb = wv; jb < (Hp >> 4); jb += SURR_THREADS / 64) {
            f32x4 acc[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] = (f32x4){0.f, 0.f, 0.f, 0.f};
            surr_gate_mac(acc, lds + m.es, m.SE, w + d.o_wih, E, Ep, H, jb, l, vec);
            if (t > 0) surr_gate_mac(acc, lds + hcur, m.SH, w + d.o_whh, H, Hp, H, jb, l, vec);      // (h0 = 0)
            const int j = jb * 16 + (l & 15);
            float bias[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) bias[q] = j < H ? w[d.o_bih + q * H + j] + w[d.o_bhh + q * H + j] : 0.f;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int r = 4 * (l >> 4) + reg;
                const float gi = surr_sigmoid(acc[0][reg] + bias[0]), gf = surr_sigmoid(acc[1][reg] + bias[1]);
                const float gg = tanhf(acc[2][reg] + bias[2]), go = surr_sigmoid(acc[3][reg] + bias[3]);
                const float c = gf * lds[m.cs + r * m.SH + j] + gi * gg;      // (a padded unit: 0.5 * 0 + 0.5 * tanh(0) = 0)
                const float h = go * tanhf(c);
                lds[m.cs + r * m.SH + j] = c;
                lds[hnext + r * m.SH + j] = h;
                if (KEEP) {
                    float* kr = kt + r * Hp + j;
                    kr[0] = gi; kr[SURR_TM * Hp] = gf; kr[2 * SURR_TM * Hp] = gg; kr[3 * SURR_TM * Hp] = go;
                    kr[SURR_KEEP_C * SURR_TM * Hp] = c; kr[SURR_KEEP_H * SURR_TM * Hp] = h;
                }
            }
        }
        __syncthreads();
        const int sw = hcur; hcur = hnext; hnext = sw;
    }
    if (tid < SURR_TM) {
        float s = 0.f;
        for (int j = 0; j < H; ++j) s = s + lds[hcur + tid * m.SH + j] * w[d.o_wo + j];
        lds[m.pr + tid] = surr_sigmoid(s + w[d.o_bo]);
    }
    __syncthreads();
    return hcur;
}

__global__ void __launch_bounds__(SURR_THREADS) k_surr_forward(const SurrDims d, const float* __restrict__ w, const float* __restrict__ x,
                                                               float* __restrict__ pred) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const SurrLds m = surr_lds(d.Ep, d.Hp, d.L, false);
    const int64_t row0 = (int64_t)blockIdx.x * SURR_TM;
    surr_forward_tile<false>(d, m, w, x, row0, lds, nullptr);
    if ((int)threadIdx.x < SURR_TM && row0 + (int)threadIdx.x < d.n) pred[row0 + threadIdx.x] = lds[m.pr + threadIdx.x];
}

// Forward, loss and backward through time of one tile.  partials: this launch's arena [tile][P]; sse: [tile] sums of squared errors
// (double: the reported loss is the float64 mean rounded once); keep: [tile][L][surr_keep_floats].  The gradient is that of the SUM of
// squared errors (dL/dpred = 2 err); k_surr_adam scales by 1/n.  Rows beyond n have err = 0 and x = 0: they contribute exactly 0.
__global__ void __launch_bounds__(SURR_THREADS) k_surr_grad(const SurrDims d, const float* __restrict__ w, const float* __restrict__ x,
                                                            const float* __restrict__ y, float* __restrict__ partials, double* __restrict__ sse,
                                                            float* __restrict__ keep_all) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const SurrLds m = surr_lds(d.Ep, d.Hp, d.L, true);
    const int tid = (int)threadIdx.x, wv = tid >> 6, l = tid & 63, li = l & 15, lk = l >> 4;
    const int E = d.E, H = d.H, Ep = d.Ep, Hp = d.Hp, n_in = d.n_in, L = d.L;
    const int64_t row0 = (int64_t)blockIdx.x * SURR_TM;
    const int64_t per_t = surr_keep_floats(Ep, Hp);
    float* keep = keep_all + (int64_t)blockIdx.x * L * per_t;
    float* part = partials + (int64_t)blockIdx.x * d.P;
    const int hlast = surr_forward_tile<true>(d, m, w, x, row0, lds, keep);

    // loss and its gradient at the prediction
    if (tid < SURR_TM) {
        const float p = lds[m.pr + tid];
        const float err = row0 + tid < d.n ? p - y[row0 + tid] : 0.f;
        lds[m.pr + 16 + tid] = (2.0f * err) * (p * (1.0f - p));
    }
    if (tid == 64) {      // (another wave than the one above: both only read pr[0..16))
        double s = 0.0;
        for (int r = 0; r < SURR_TM; ++r)
            if (row0 + r < d.n) { const double e = (double)lds[m.pr + r] - (double)y[row0 + r]; s += e * e; }
        sse[blockIdx.x] = s;
    }
    __syncthreads();
    const float* dz = lds + m.pr + 16;
    for (int j = tid; j < H; j += SURR_THREADS) {
        float s = 0.f;
        for (int r = 0; r < SURR_TM; ++r) s = s + dz[r] * lds[hlast + r * m.SH + j];
        part[d.o_wo + j] = s;
    }
    if (tid == SURR_THREADS - 1) {
        float s = 0.f;
        for (int r = 0; r < SURR_TM; ++r) s = s + dz[r];
        part[d.o_bo] = s;
    }
    for (int i = tid; i < SURR_TM * Hp; i += SURR_THREADS) {
        const int r = i / Hp, j = i - r * Hp;
        lds[m.dh + r * m.SH + j] = j < H ? dz[r] * w[d.o_wo + j] : 0.f;
        lds[m.dc + r * m.SH + j] = 0.f;
    }
    __syncthreads();

    for (int t = L - 1; t >= 0; --t) {
        float* kt = keep + t * per_t;
        // the cell backwards (elementwise): pre-activation gate gradients into LDS and over the kept gates
        for (int i = tid; i < SURR_TM * Hp; i += SURR_THREADS) {
            const int r = i / Hp, j = i - r * Hp;
            float* kr = kt + i;
            const float gi = kr[0], gf = kr[SURR_TM * Hp], gg = kr[2 * SURR_TM * Hp], go = kr[3 * SURR_TM * Hp];
            const float c = kr[SURR_KEEP_C * SURR_TM * Hp];
            const float cprev = t > 0 ? kr[SURR_KEEP_C * SURR_TM * Hp - per_t] : 0.f;
            const float dh = lds[m.dh + r * m.SH + j];
            const float tc = tanhf(c);
            const float dc = lds[m.dc + r * m.SH + j] + (dh * go) * (1.0f - tc * tc);
            const float di = (dc * gg) * (gi * (1.0f - gi)), df = (dc * cprev) * (gf * (1.0f - gf));
            const float dg = (dc * gi) * (1.0f - gg * gg), dO = (dh * tc) * (go * (1.0f - go));
            lds[m.dc + r * m.SH + j] = dc * gf;
            float* g = lds + m.dgs + r * m.SG + j;
            g[0] = di; g[Hp] = df; g[2 * Hp] = dg; g[3 * Hp] = dO;
            kr[0] = di; kr[SURR_TM * Hp] = df; kr[2 * SURR_TM * Hp] = dg; kr[3 * SURR_TM * Hp] = dO;
        }
        __syncthreads();
        // dh_{t-1} = dgates Whh (t > 0), de_t = dgates Wih (MFMA, contraction over the 4 H gate columns), then through the embedding's sigmoid
        const int nH = t > 0 ? (Hp >> 4) : 0, nO = nH + (Ep >> 4);
        for (int ot = wv; ot < nO; ot += SURR_THREADS / 64) {
            const bool to_h = ot < nH;
            const int ld = to_h ? H : E, col = (to_h ? ot : ot - nH) * 16 + li;
            const float* W = w + (to_h ? d.o_whh : d.o_wih);
            const bool colok = col < ld;
            f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
            for (int q = 0; q < 4; ++q)
                for (int j16 = 0; j16 < Hp; j16 += 16) {
                    const f32x4 a = *reinterpret_cast<const f32x4*>(lds + m.dgs + li * m.SG + q * Hp + j16 + 4 * lk);
                    float b[4];
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const int jj = j16 + 4 * lk + s;
                        b[s] = (colok && jj < H) ? W[(int64_t)(q * H + jj) * ld + col] : 0.f;
                    }
                    acc0 = MFMA16(a[0], b[0], acc0);
                    acc1 = MFMA16(a[1], b[1], acc1);
                    acc0 = MFMA16(a[2], b[2], acc0);
                    acc1 = MFMA16(a[3], b[3], acc1);
                }
            const f32x4 acc = acc0 + acc1;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int r = 4 * lk + reg;
                if (to_h) lds[m.dh + r * m.SH + col] = acc[reg];
                else {
                    const float e = kt[6 * SURR_TM * Hp + r * Ep + col];
                    lds[m.dps + (t * SURR_TM + r) * m.SE + col] = acc[reg] * (e * (1.0f - e));
                }
            }
        }
        __syncthreads();
    }

    // weight gradients: dWih[gate row][k] = sum_t sum_r dgates_t[r][gate row] e_t[r][k]; dWhh with h_{t-1} (t >= 1).  One 16 x 16
    // output tile per wave and pass, contraction over the 16 rows of every step (MFMA); operands come back from the tile's scratch.
    {
        const int nkE = Ep >> 4, nk = nkE + (Hp >> 4), nhb = Hp >> 4, total = 4 * nhb * nk;
        for (int ot = wv; ot < total; ot += SURR_THREADS / 64) {
            const int gt = ot / nk, kb = ot - gt * nk, q = gt / nhb, jb = gt - q * nhb;
            const bool ih = kb < nkE;
            const int ldp = ih ? Ep : Hp, ld = ih ? E : H, kc = (ih ? kb : kb - nkE) * 16 + li;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            for (int t = ih ? 0 : 1; t < L; ++t) {
                const float* ga = keep + t * per_t + q * SURR_TM * Hp + jb * 16 + li;
                const float* sb = ih ? keep + t * per_t + 6 * SURR_TM * Hp + kc : keep + (t - 1) * per_t + SURR_KEEP_H * SURR_TM * Hp + kc;
#pragma unroll
                for (int r4 = 0; r4 < 4; ++r4) acc = MFMA16(ga[(4 * r4 + lk) * Hp], sb[(4 * r4 + lk) * ldp], acc);
            }
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int jj = jb * 16 + 4 * lk + reg;
                if (jj < H && kc < ld) part[(ih ? d.o_wih : d.o_whh) + (int64_t)(q * H + jj) * ld + kc] = acc[reg];
            }
        }
    }
    // the two LSTM biases share one gradient (written twice, bit for bit)
    for (int gc = tid; gc < 4 * Hp; gc += SURR_THREADS) {
        const int q = gc / Hp, jj = gc - q * Hp;
        if (jj < H) {
            float s = 0.f;
            for (int t = 0; t < L; ++t)
                for (int r = 0; r < SURR_TM; ++r) s = s + keep[t * per_t + q * SURR_TM * Hp + r * Hp + jj];
            part[d.o_bih + q * H + jj] = s;
            part[d.o_bhh + q * H + jj] = s;
        }
    }
    // the embedding (VALU)
    for (int i = tid; i < E * (n_in + 1); i += SURR_THREADS) {
        const int j = i / (n_in + 1), k = i - j * (n_in + 1);
        float s = 0.f;
        for (int t = 0; t < L; ++t)
            for (int r = 0; r < SURR_TM; ++r) {
                const float dp = lds[m.dps + (t * SURR_TM + r) * m.SE + j];
                s = s + (k < n_in ? dp * lds[m.xs + (t * SURR_TM + r) * SURR_MAX_IN + k] : dp);
            }
        part[k < n_in ? j * n_in + k : d.o_be + j] = s;
    }
}

// One thread per parameter: g = (partials of tile 0 + tile 1 + ...) / n, then torch.optim.Adam (foreach=False form).  The moments are
// adam1's float32 statements (common.hip.h): g += wd w; m += (1 - b1)(g - m); v = v b2 + ((1 - b2) g) g.  The parameter update
// w -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps) is evaluated in float64 on those float32 moments and rounded ONCE: seven float32
// roundings of a step of size lr reach 2-4 ulp of a parameter near zero (|w| << lr), and the update is held to 2 ulp of |w| + lr of
// the float64 formula (tests/test_gpu_surrogate_engine.py); 81,301 float64 divisions per step cost nothing next to k_surr_grad.
// Thread 0 also leaves the step's loss (computed BEFORE this update): the float64 mean of the tiles' squared errors, rounded once.
struct SurrAdam { double ss, bc2s, eps; float w1, b2, w2, wd; };      // ss = lr / bc1, bc2s = sqrt(bc2), w1 = 1 - b1, w2 = 1 - b2
__global__ void __launch_bounds__(SURR_THREADS) k_surr_adam(float* __restrict__ w, float* __restrict__ m, float* __restrict__ v,
                                                            const float* __restrict__ partials, const double* __restrict__ sse, const int ntiles,
                                                            const int P, const float inv_n, const double n, const SurrAdam c, float* __restrict__ loss) {
    const int p = (int)(blockIdx.x * SURR_THREADS + threadIdx.x);
    if (p == 0) {
        double s = 0.0;
        for (int t = 0; t < ntiles; ++t) s += sse[t];
        *loss = (float)(s / n);
    }
    if (p >= P) return;
    float g = partials[p];
    for (int t = 1; t < ntiles; ++t) g = g + partials[(int64_t)t * P + p];
    g = g * inv_n;
    const float w0 = w[p];
    float m1 = m[p], v1 = v[p];
    g = g + c.wd * w0;
    m1 = m1 + c.w1 * (g - m1);
    v1 = v1 * c.b2;
    v1 = v1 + (c.w2 * g) * g;
    const double denom = sqrt((double)v1) / c.bc2s + c.eps;
    w[p] = (float)((double)w0 - c.ss * ((double)m1 / denom));
    m[p] = m1; v[p] = v1;
}

// ------------------------------------------------------------------------------------------------
// Host side.  Stateless: the caller owns every buffer; the calls run on the calling thread's current device.
// ------------------------------------------------------------------------------------------------
static std::string surr_num(const double v) {
    char buf[40];
    snprintf(buf, sizeof(buf), "%g", v);
    return buf;
}
static int surr_check_shape(const mfas_surrogate_shape* s) {
    if (!s) return fail(MFAS_EINVAL, "surrogate: null shape");
    if (s->n_in < 1 || s->n_in > SURR_MAX_IN) return fail(MFAS_EINVAL, "surrogate: n_in = " + std::to_string(s->n_in) + " outside 1..8");
    if (s->E < 16 || s->E > 128) return fail(MFAS_EINVAL, "surrogate: E = " + std::to_string(s->E) + " outside 16..128");
    if (s->H < 16 || s->H > 128) return fail(MFAS_EINVAL, "surrogate: H = " + std::to_string(s->H) + " outside 16..128");
    return MFAS_OK;
}
static int surr_check_bucket(const int32_t L, const int64_t n) {
    if (L < 1 || L > MFAS_MAX_CELLS) return fail(MFAS_EINVAL, "surrogate: L = " + std::to_string(L) + " outside 1.." + std::to_string(MFAS_MAX_CELLS));
    if (n < 1 || n > SURR_MAX_ROWS) return fail(MFAS_EINVAL, "surrogate: n = " + std::to_string(n) + " outside 1.." + std::to_string(SURR_MAX_ROWS));
    return MFAS_OK;
}

static SurrDims surr_dims(const mfas_surrogate_shape& s, const int32_t L, const int64_t n, const void* params) {
    SurrDims d;
    memset(&d, 0, sizeof(d));
    d.n_in = s.n_in; d.E = s.E; d.H = s.H; d.Ep = (s.E + 15) & ~15; d.Hp = (s.H + 15) & ~15; d.L = L; d.n = n;
    d.o_be = s.E * s.n_in;
    d.o_wih = d.o_be + s.E;
    d.o_whh = d.o_wih + 4 * s.H * s.E;
    d.o_bih = d.o_whh + 4 * s.H * s.H;
    d.o_bhh = d.o_bih + 4 * s.H;
    d.o_wo = d.o_bhh + 4 * s.H;
    d.o_bo = d.o_wo + s.H;
    d.P = d.o_bo + 1;
    d.vec = (s.E % 4 == 0 && s.H % 4 == 0 && d.o_wih % 4 == 0 && (reinterpret_cast<uintptr_t>(params) & 15) == 0) ? 1 : 0;
    return d;
}

// scratch of one bucket: [loss | pad to 256 B][sse: T doubles][partials: T x P floats][kept steps: T x L x surr_keep_floats], T = tiles
struct SurrScratch { int64_t tiles, o_sse, o_part, o_keep, bytes; };
static SurrScratch surr_scratch(const SurrDims& d) {
    auto up = [](int64_t b) { return (b + 255) & ~int64_t(255); };
    SurrScratch s;
    s.tiles = (d.n + SURR_TM - 1) / SURR_TM;
    s.o_sse = 256;
    s.o_part = up(s.o_sse + 8 * s.tiles);
    s.o_keep = up(s.o_part + 4 * s.tiles * d.P);
    s.bytes = up(s.o_keep + 4 * s.tiles * d.L * surr_keep_floats(d.Ep, d.Hp));
    return s;
}

extern "C" int64_t mfas_surrogate_param_count(const mfas_surrogate_shape* shape) {
    if (int rc = surr_check_shape(shape)) return rc;
    return surr_dims(*shape, 1, 1, nullptr).P;
}

extern "C" int64_t mfas_surrogate_scratch_bytes(const mfas_surrogate_shape* shape, int32_t max_L, int64_t max_n) {
    if (int rc = surr_check_shape(shape)) return rc;
    if (int rc = surr_check_bucket(max_L, max_n)) return rc;
    return surr_scratch(surr_dims(*shape, max_L, max_n, nullptr)).bytes;
}

extern "C" int mfas_surrogate_train(const mfas_surrogate_shape* shape, float* params, float* exp_avg, float* exp_avg_sq, int64_t* step,
                                    const float* const* x, const float* const* y, const int32_t* L, const int64_t* n, int32_t n_buckets,
                                    int32_t epochs, double lr, double beta1, double beta2, double eps, double weight_decay, void* scratch,
                                    int64_t scratch_bytes, void* hip_stream, float* last_loss) {
    if (int rc = surr_check_shape(shape)) return rc;
    if (!params || !exp_avg || !exp_avg_sq || !step || !x || !y || !L || !n || !scratch || !last_loss)
        return fail(MFAS_EINVAL, "surrogate_train: null pointer");
    if (n_buckets < 1) return fail(MFAS_EINVAL, "surrogate_train: n_buckets = " + std::to_string(n_buckets) + " < 1");
    if (epochs < 1) return fail(MFAS_EINVAL, "surrogate_train: epochs = " + std::to_string(epochs) + " < 1");
    if (*step < 0) return fail(MFAS_EINVAL, "surrogate_train: step = " + std::to_string(*step) + " < 0");
    if (!(beta1 >= 0.0 && beta1 < 1.0)) return fail(MFAS_EINVAL, "surrogate_train: beta1 = " + surr_num(beta1) + " outside [0, 1)");
    if (!(beta2 >= 0.0 && beta2 < 1.0)) return fail(MFAS_EINVAL, "surrogate_train: beta2 = " + surr_num(beta2) + " outside [0, 1)");
    if (!(eps >= 0.0)) return fail(MFAS_EINVAL, "surrogate_train: eps = " + surr_num(eps) + " < 0");
    if (reinterpret_cast<uintptr_t>(scratch) & 15) return fail(MFAS_EINVAL, "surrogate_train: scratch is not 16-byte aligned");
    int maxL = 1;
    for (int b = 0; b < n_buckets; ++b) {
        if (int rc = surr_check_bucket(L[b], n[b])) return rc;
        if (!x[b] || !y[b]) return fail(MFAS_EINVAL, "surrogate_train: null pointer (bucket " + std::to_string(b) + ")");
        const int64_t need = surr_scratch(surr_dims(*shape, L[b], n[b], params)).bytes;
        if (scratch_bytes < need)
            return fail(MFAS_EINVAL, "surrogate_train: scratch_bytes = " + std::to_string(scratch_bytes) + " < " + std::to_string(need) +
                                         " (mfas_surrogate_scratch_bytes, bucket " + std::to_string(b) + ")");
        maxL = std::max(maxL, (int)L[b]);
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    const SurrDims dmax = surr_dims(*shape, maxL, 1, params);
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_surr_grad), hipFuncAttributeMaxDynamicSharedMemorySize,
                               surr_lds(dmax.Ep, dmax.Hp, maxL, true).total * 4));
    char* base = static_cast<char*>(scratch);
    float* d_loss = reinterpret_cast<float*>(base);
    int64_t t = *step;
    for (int ep = 0; ep < epochs; ++ep)
        for (int b = 0; b < n_buckets; ++b) {
            const SurrDims d = surr_dims(*shape, L[b], n[b], params);
            const SurrScratch sc = surr_scratch(d);
            double* sse = reinterpret_cast<double*>(base + sc.o_sse);
            float* part = reinterpret_cast<float*>(base + sc.o_part);
            float* keep = reinterpret_cast<float*>(base + sc.o_keep);
            ++t;
            SurrAdam c;
            c.ss = lr / (1.0 - std::pow(beta1, (double)t));
            c.bc2s = std::sqrt(1.0 - std::pow(beta2, (double)t));
            c.eps = eps;
            c.w1 = (float)(1.0 - beta1); c.b2 = (float)beta2; c.w2 = (float)(1.0 - beta2); c.wd = (float)weight_decay;
            hipLaunchKernelGGL(k_surr_grad, dim3((unsigned)sc.tiles), dim3(SURR_THREADS), (size_t)surr_lds(d.Ep, d.Hp, d.L, true).total * 4, st,
                               d, (const float*)params, x[b], y[b], part, sse, keep);
            hipLaunchKernelGGL(k_surr_adam, dim3((unsigned)((d.P + SURR_THREADS - 1) / SURR_THREADS)), dim3(SURR_THREADS), 0, st, params, exp_avg,
                               exp_avg_sq, (const float*)part, (const double*)sse, (int)sc.tiles, d.P, (float)(1.0 / (double)d.n), (double)d.n, c, d_loss);
        }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(last_loss, d_loss, sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    *step = t;
    return MFAS_OK;
}

extern "C" int mfas_surrogate_forward(const mfas_surrogate_shape* shape, const float* params, const float* x, int32_t L, int64_t n, float* pred,
                                      void* scratch, int64_t scratch_bytes, void* hip_stream) {
    (void)scratch; (void)scratch_bytes;      // the forward keeps nothing between its steps outside LDS
    if (int rc = surr_check_shape(shape)) return rc;
    if (!params || !x || !pred) return fail(MFAS_EINVAL, "surrogate_forward: null pointer");
    if (int rc = surr_check_bucket(L, n)) return rc;
    const SurrDims d = surr_dims(*shape, L, n, params);
    const size_t lds = (size_t)surr_lds(d.Ep, d.Hp, d.L, false).total * 4;
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_surr_forward), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_surr_forward, dim3((unsigned)((n + SURR_TM - 1) / SURR_TM)), dim3(SURR_THREADS), lds, reinterpret_cast<hipStream_t>(hip_stream),
                       d, params, x, pred);
    HIPCHK(hipGetLastError());
    return MFAS_OK;
}
