// Audio front end (DESIGN.md 23): the amplitude envelope and the onset detector behind the model's `onset+amplitude` input and the beat
// consistency's audio side - what the reference takes from numpy stride tricks and librosa.onset.onset_detect (dataloaders/beat_sep_lower.py:391-409,
// utils/metric.py:64-76).  Included by syn_kernels.hip.
//
// Several takes of different lengths share every launch: y [total samples] fp32 is the takes back to back, sample_off / frame_off [n_takes + 1]
// int64 on the device are their starts (frames of take i: T_i = 1 + n_i / hop).  Nothing of a take depends on its batch mates: every take-wide
// quantity (the dB floor, the envelope's min and max) is reduced per take, no atomics, every sum in the order written here.
//
//   k_power      P[t][k] = |sum_j w[j] ypad[t hop + j] e^{-2 pi i jk / 2048}|^2, fp64: a GEMM of 16-frame row tiles against the [cos | -sin] basis on
//                v_mfma_f64_16x16x4_f64.  A workgroup owns a row tile (or, where there are few, one of 2 / 4 / 8 shares of its column tiles) and its
//                four waves walk the 65 column tiles of 16 bins (bin 1024 is alone in the last); a sum over j is two chains, even and odd steps
//                of four samples, added at the end.  The tile's samples sit in the LDS once, as fp32 (the 16 frames overlap: 15 hop + 2048 samples), and become fp64
//                operands on the way into the MFMA: (double)y * w[j], one multiply, w[j] = 0.5 - 0.5 cos(2 pi j / 2048).  The basis is a 2048-entry
//                fp64 table cos(2 pi i / 2048) in the LDS, filled by cospi on exact arguments (i / 1024), gathered at i = jk mod 2048 - the
//                integer product reduced exactly - and at i + 512 for -sin.  Both chains of a bin end in the same lane: P = re re + im im there.
//   k_mel_db     S[t][m] = 10 log10(max(1e-10, sum_k W[m][k] P[t][k])): a thread per (t, m), k ascending over the filter's support, the Slaney
//                weights from the 130 edge frequencies (computed on the host in fp64, passed by value).
//   k_db_floor   S = max(S, max over the take - 80): a workgroup per take.
//   k_flux       env[t] = t < lag ? 0 : (sum_{m = 0..127, ascending} max(0, S[t - lag + 1][m] - S[t - lag][m])) / 128, lag = 1 + 2048 / (2 hop) (3 at
//                hop 512): 16 frames a workgroup, rows through the LDS.
//   k_env_norm   x = (env - min) / (max - min + FLT_MIN): a workgroup per take.
//   k_peak_pick  a workgroup per take: every frame's two window tests in parallel (the mean: a sum in ascending frame order over the truncated window,
//                divided by its length), then - with wait > 0 - one lane walks the candidates in order and enforces `wait`.
//   k_amplitude  a[i] = max |y[i .. i + L)|: per block of L outputs a suffix maximum over the block and a prefix maximum over the next one
//                (two scans in the LDS), a[i] = max(suffix[i], prefix[i - 1]); k_amp_tail repeats a[n - L] over the last L - 1 entries.
namespace {
namespace audio {

constexpr int kNfft = 2048, kBins = kNfft / 2 + 1, kMels = 128, kRowTile = 16, kColTiles = (kBins + 15) / 16, kMaxFrameLength = 4096;
constexpr int kTableBytes = kNfft * 8;
typedef double d4 __attribute__((ext_vector_type(4)));

// Sample i of a row tile's span sits at i + i / 128 in the LDS: the 16 rows of an A fragment are hop samples apart, and a hop of 512 (any multiple of
// 64) would put them all into one bank; with the skew, rows 512 apart are 4 banks apart and a fragment load of hop 512 touches 64 different banks.
__device__ __host__ inline int skew(int i) { return i + (i >> 7); }
static int power_lds(int hop) { return kTableBytes + (skew(15 * hop + kNfft) + 1) * 4; }

struct PowerArgs {
    const float* y; const long long* soff; const long long* foff;
    double* P;
    int hop;
};

__global__ __launch_bounds__(256) void k_power(const PowerArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem_audio[];
    double* tab = reinterpret_cast<double*>(smem_audio);                       // cos(2 pi i / 2048)
    float* span = reinterpret_cast<float*>(smem_audio + kTableBytes);          // ypad[t0 hop .. t0 hop + 15 hop + 2048)
    const int take = blockIdx.y, tid = threadIdx.x;
    const long long y0 = a.soff[take], n = a.soff[take + 1] - y0, f0 = a.foff[take], T = a.foff[take + 1] - f0;
    const long long t0 = (long long)blockIdx.x * kRowTile;
    if (t0 >= T) return;
    const int hop = a.hop, nspan = 15 * hop + kNfft;
    for (int i = tid; i < nspan; i += 256) {
        const long long s = t0 * hop + i - kNfft / 2;                          // centred frames: 1024 zeros in front of the take and behind it
        span[skew(i)] = (s >= 0 && s < n) ? a.y[y0 + s] : 0.f;
    }
    for (int i = tid; i < kNfft; i += 256) tab[i] = cospi((double)i * (1.0 / 1024.0));
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63, r = lane & 15, q = lane >> 4;
    const int abase = r * hop + q;                                             // A[row r][j = 4 s + q] = span sample r hop + j
    for (int ct = blockIdx.z * 4 + wave; ct < kColTiles; ct += 4 * gridDim.z) {      // gridDim.z workgroups share a row tile's column tiles
        const unsigned bin = ct * 16 + r;                                      // B[j = 4 s + q][column r]; bins past 1024 are computed and dropped
        const unsigned step = (4u * bin) & (kNfft - 1);
        unsigned idx = ((unsigned)q * bin) & (kNfft - 1);                      // (j bin) mod 2048, carried from step to step
        // two chains per sum, even and odd steps (a chain's MFMAs wait for each other), added at the end: re = re_even + re_odd
        d4 re = {0.0, 0.0, 0.0, 0.0}, im = {0.0, 0.0, 0.0, 0.0}, re1 = {0.0, 0.0, 0.0, 0.0}, im1 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 2
        for (int s = 0; s < kNfft / 4; s += 2) {
            const double w0 = __builtin_fma(-0.5, tab[4 * s + q], 0.5), w1 = __builtin_fma(-0.5, tab[4 * s + 4 + q], 0.5);
            const double a0 = (double)span[skew(abase + 4 * s)] * w0, a1 = (double)span[skew(abase + 4 * s + 4)] * w1;
            const unsigned idx1 = (idx + step) & (kNfft - 1);
            const double c0 = tab[idx], s0 = tab[(idx + kNfft / 4) & (kNfft - 1)];  // cos(x + pi / 2) = -sin x
            const double c1 = tab[idx1], s1 = tab[(idx1 + kNfft / 4) & (kNfft - 1)];
            re = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, c0, re, 0, 0, 0);
            im = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, s0, im, 0, 0, 0);
            re1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, c1, re1, 0, 0, 0);
            im1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, s1, im1, 0, 0, 0);
            idx = (idx1 + step) & (kNfft - 1);
        }
        re += re1;
        im += im1;
#pragma unroll
        for (int i = 0; i < 4; ++i) {                                          // C/D of the f64 form: column = lane & 15, row = (lane >> 4) + 4 i
            const long long t = t0 + q + 4 * i;
            if (t < T && bin < (unsigned)kBins) a.P[(f0 + t) * kBins + bin] = __builtin_fma(im[i], im[i], re[i] * re[i]);
        }
    }
}

struct MelArgs {
    const double* P; double* S;
    long long rows;                  // frames of all takes
    double df;                       // sr / 2048
    double f[kMels + 2];             // the Slaney edge frequencies
};

__global__ __launch_bounds__(256) void k_mel_db(const MelArgs a) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.rows * kMels) return;
    const long long t = idx / kMels;
    const int m = (int)(idx - t * kMels);
    const double f0 = a.f[m], f1 = a.f[m + 1], f2 = a.f[m + 2], norm = 2.0 / (f2 - f0);
    int k_lo = (int)(f0 / a.df) - 1, k_hi = (int)(f2 / a.df) + 1;              // a bin more on either side: its weight is max(0, negative) = 0
    k_lo = k_lo < 0 ? 0 : k_lo;
    k_hi = k_hi > kBins - 1 ? kBins - 1 : k_hi;
    const double* __restrict__ p = a.P + t * kBins;
    double acc = 0.0;
    for (int k = k_lo; k <= k_hi; ++k) {
        const double fk = k * a.df, lower = (fk - f0) / (f1 - f0), upper = (f2 - fk) / (f2 - f1);
        const double w = fmax(0.0, fmin(lower, upper)) * norm;
        acc = __builtin_fma(w, p[k], acc);
    }
    a.S[idx] = 10.0 * log10(fmax(1e-10, acc));
}

constexpr int kWide = 1024;          // threads of the workgroup-per-take kernels

// max over the kWide threads' values, handed to all of them (order-free)
__device__ inline double block_max(double v, double* s) {
    const int tid = threadIdx.x;
    __syncthreads();
    s[tid] = v;
    __syncthreads();
    for (int d = kWide / 2; d > 0; d >>= 1) {
        if (tid < d) s[tid] = fmax(s[tid], s[tid + d]);
        __syncthreads();
    }
    return s[0];
}

__global__ __launch_bounds__(kWide) void k_db_floor(double* S, const long long* foff, double top_db) {
    __shared__ double s[kWide];
    const long long b = foff[blockIdx.x] * kMels, e = foff[blockIdx.x + 1] * kMels;
    double m = -__builtin_inf();
    for (long long i = b + threadIdx.x; i < e; i += kWide) m = fmax(m, S[i]);
    const double floor_db = block_max(m, s) - top_db;
    for (long long i = b + threadIdx.x; i < e; i += kWide) S[i] = fmax(S[i], floor_db);
}

// env of 16 frames of a take per workgroup: their 17 rows of S through the LDS (coalesced reads), then a thread per frame adds its 128 bands in order
constexpr int kFluxFrames = 16, kFluxPitch = kMels + 1;
__global__ __launch_bounds__(128) void k_flux(const double* S, const long long* foff, int lag, double* env) {
    __shared__ double rows[(kFluxFrames + 1) * kFluxPitch];
    const long long f0 = foff[blockIdx.y], T = foff[blockIdx.y + 1] - f0, t0 = (long long)blockIdx.x * kFluxFrames;
    if (t0 >= T) return;
    const int tid = threadIdx.x;
    for (int i = 0; i <= kFluxFrames; ++i) {                                   // row i = frame t0 + i - lag: the earlier row of env[t0 + i]
        const long long t = t0 + i - lag;
        rows[i * kFluxPitch + tid] = (t >= 0 && t < T) ? S[(f0 + t) * kMels + tid] : 0.0;
    }
    __syncthreads();
    if (tid < kFluxFrames && t0 + tid < T) {
        double e = 0.0;
        if (t0 + tid >= lag) {
            const double* a = rows + tid * kFluxPitch;
            for (int m = 0; m < kMels; ++m) e += fmax(0.0, a[kFluxPitch + m] - a[m]);
            e /= (double)kMels;
        }
        env[f0 + t0 + tid] = e;
    }
}

__global__ __launch_bounds__(kWide) void k_env_norm(const long long* foff, const double* env, double* env_norm) {
    __shared__ double s[kWide];
    const long long f0 = foff[blockIdx.x], T = foff[blockIdx.x + 1] - f0;
    double lo = __builtin_inf(), hi = -__builtin_inf();
    for (long long t = threadIdx.x; t < T; t += kWide) {
        const double e = env[f0 + t];
        lo = fmin(lo, e);
        hi = fmax(hi, e);
    }
    lo = -block_max(-lo, s);
    hi = block_max(hi, s);
    const double scale = (hi - lo) + 1.1754943508222875e-38;
    for (long long t = threadIdx.x; t < T; t += kWide) env_norm[f0 + t] = (env[f0 + t] - lo) / scale;
}

struct PeakArgs {
    const double* x; const double* raw; const long long* foff;
    unsigned char* mask; int* count;
    int pre_max, post_max, pre_avg, post_avg, wait;
    double delta;
};

__global__ __launch_bounds__(256) void k_peak_pick(const PeakArgs a) {
    __shared__ int s_n[256];
    const long long f0 = a.foff[blockIdx.x], T = a.foff[blockIdx.x + 1] - f0;
    const int lane = threadIdx.x;
    const double* __restrict__ x = a.x + f0;
    unsigned char* mask = a.mask + f0;
    bool live = true;
    if (a.raw) {                                                               // an envelope that is zero everywhere has no onsets, whatever delta
        int any = 0;
        for (long long t = lane; t < T; t += 256) any |= a.raw[f0 + t] != 0.0;
        live = __syncthreads_or(any) != 0;
    }
    int mine = 0;
    for (long long i = lane; i < T; i += 256) {
        bool peak = live;
        if (peak) {
            const long long b = i - a.pre_max < 0 ? 0 : i - a.pre_max, e = i + a.post_max > T ? T : i + a.post_max;
            double mx = x[i];
            for (long long j = b; j < e; ++j) mx = fmax(mx, x[j]);
            peak = x[i] == mx;
        }
        if (peak) {
            const long long b = i - a.pre_avg < 0 ? 0 : i - a.pre_avg, e = i + a.post_avg > T ? T : i + a.post_avg;
            double sum = 0.0;
            for (long long j = b; j < e; ++j) sum += x[j];
            peak = x[i] >= sum / (double)(e - b) + a.delta;
        }
        mask[i] = peak ? 1 : 0;
        mine += peak ? 1 : 0;
    }
    s_n[lane] = mine;
    __syncthreads();                                                           // the candidates are written (global and LDS writes of the workgroup)
    if (a.wait == 0) {                                                         // no waiting: every candidate is an onset
        for (int d = 128; d > 0; d >>= 1) {
            if (lane < d) s_n[lane] += s_n[lane + d];
            __syncthreads();
        }
        if (lane == 0) a.count[blockIdx.x] = s_n[0];
    } else if (lane == 0) {
        int n = 0;
        long long last = -1 - (long long)a.wait;
        for (long long i = 0; i < T; ++i) {
            if (!mask[i]) continue;
            if (i - last > a.wait) { last = i; ++n; } else mask[i] = 0;
        }
        a.count[blockIdx.x] = n;
    }
}

// block bx of a take: outputs [bx L, bx L + L) that exist (i <= n - L)
__global__ __launch_bounds__(256) void k_amplitude(const float* y, const long long* soff, int L, float* out) {
    extern __shared__ __attribute__((aligned(16))) char smem_audio[];
    float* buf0 = reinterpret_cast<float*>(smem_audio);                        // [0, L): this block, [L, 2 L): the next
    float* buf1 = buf0 + 2 * L;
    const int tid = threadIdx.x;
    const long long s0 = soff[blockIdx.y], n = soff[blockIdx.y + 1] - s0, base = (long long)blockIdx.x * L;
    if (n < L || base > n - L) return;
    for (int i = tid; i < 2 * L; i += 256) buf0[i] = base + i < n ? fabsf(y[s0 + base + i]) : 0.f;
    __syncthreads();
    float* src = buf0;
    float* dst = buf1;
    for (int d = 1; d < L; d <<= 1) {
        for (int i = tid; i < L; i += 256) {
            dst[i] = i + d < L ? fmaxf(src[i], src[i + d]) : src[i];                       // suffix maximum
            dst[L + i] = i - d >= 0 ? fmaxf(src[L + i], src[L + i - d]) : src[L + i];      // prefix maximum
        }
        __syncthreads();
        float* t = src; src = dst; dst = t;
    }
    for (int i = tid; i < L; i += 256)
        if (base + i <= n - L) out[s0 + base + i] = i ? fmaxf(src[i], src[L + i - 1]) : src[0];
}

__global__ __launch_bounds__(256) void k_amp_tail(const long long* soff, int L, float* out) {
    const long long s0 = soff[blockIdx.y], n = soff[blockIdx.y + 1] - s0;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (n < L || i >= L - 1) return;
    out[s0 + n - L + 1 + i] = out[s0 + n - L];
}

// the 130 edge frequencies: equally spaced on the Slaney mel scale between 0 and sr / 2
static void mel_edges(double sr, double* f) {
    const double f_sp = 200.0 / 3.0, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = log(6.4) / 27.0;
    const double nyq = 0.5 * sr, top = nyq >= min_log_hz ? min_log_mel + log(nyq / min_log_hz) / logstep : nyq / f_sp;
    for (int i = 0; i < kMels + 2; ++i) {
        const double mel = top * (double)i / (double)(kMels + 1);
        f[i] = mel >= min_log_mel ? min_log_hz * exp(logstep * (mel - min_log_mel)) : f_sp * mel;
    }
    f[kMels + 1] = nyq;
}

static const char* bad_batch(const void* y, const void* soff, const void* foff, int32_t n_takes, int64_t max_frames, int64_t total_frames, int32_t hop) {
    if (!y || !soff || !foff) return "null pointer";
    if (n_takes < 1 || n_takes > 65535) return "1 to 65535 takes a call";
    if (hop < 1 || hop > kNfft) return "hop is 1 to 2048";
    if (max_frames < 1 || total_frames < max_frames || total_frames > (1LL << 40)) return "frame counts: 1 <= max_frames <= total_frames";
    if ((max_frames + kRowTile - 1) / kRowTile > 0x7fffffffLL) return "too many frames in a take for one launch";
    return nullptr;
}

static int launch_power(const float* y, const int64_t* soff, const int64_t* foff, int32_t n_takes, int64_t max_frames, int32_t hop, double* P, hipStream_t s) {
    static OncePerDevice once;
    if (once.first()) allow_lds(k_power, power_lds(kNfft));
    PowerArgs a = {};
    a.y = y; a.soff = (const long long*)soff; a.foff = (const long long*)foff; a.P = P; a.hop = hop;
    // column groups: enough workgroups for four per CU on a 256-CU chip where the row tiles alone are fewer (a tile's arithmetic does not depend on the split)
    const int64_t row_tiles = (max_frames + kRowTile - 1) / kRowTile * n_takes;
    int groups = 1;
    while (groups < 8 && row_tiles * groups < 1024) groups *= 2;
    hipLaunchKernelGGL(k_power, dim3((unsigned)((max_frames + kRowTile - 1) / kRowTile), n_takes, groups), dim3(256), power_lds(hop), s, a);
    return launched("k_power launch");
}

}  // namespace audio
}  // namespace

// ---- entry points -----------------------------------------------------------------------------------------------------------------------------------
extern "C" {

int64_t syn_audio_workspace_bytes(int64_t total_frames) {
    if (total_frames < 1 || total_frames > (1LL << 40)) return -1;
    return total_frames * audio::kBins * 8;
}

int syn_audio_amplitude(const float* y, const int64_t* sample_off, int32_t n_takes, int64_t max_samples, int32_t frame_length, float* out, void* stream) {
    if (!y || !sample_off || !out) return fail_msg("syn_audio_amplitude: null pointer");
    if (n_takes < 1 || n_takes > 65535) return fail_msg("syn_audio_amplitude: 1 to 65535 takes a call");
    if (frame_length < 1 || frame_length > audio::kMaxFrameLength) return fail_msg("syn_audio_amplitude: frame_length is 1 to 4096");
    if (max_samples < frame_length) return fail_msg("syn_audio_amplitude: a take is at least frame_length samples");
    const int64_t blocks = (max_samples - frame_length) / frame_length + 1;
    if (blocks > 0x7fffffffLL) return fail_msg("syn_audio_amplitude: too many samples in a take for one launch");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(audio::k_amplitude, dim3((unsigned)blocks, n_takes), dim3(256), 16 * frame_length, s, y, (const long long*)sample_off, (int)frame_length, out);
    if (frame_length > 1)
        hipLaunchKernelGGL(audio::k_amp_tail, dim3((unsigned)((frame_length + 254) / 256), n_takes), dim3(256), 0, s, (const long long*)sample_off, (int)frame_length, out);
    return launched("k_amplitude launches");
}

int syn_audio_power_spectrum(const float* y, const int64_t* sample_off, const int64_t* frame_off, int32_t n_takes, int64_t max_frames, int64_t total_frames,
                             int32_t hop, double* power, void* stream) {
    if (const char* why = audio::bad_batch(y, sample_off, frame_off, n_takes, max_frames, total_frames, hop)) {
        snprintf(g_err, sizeof(g_err), "syn_audio_power_spectrum: %s", why);
        return -2;
    }
    if (!power) return fail_msg("syn_audio_power_spectrum: null pointer");
    return audio::launch_power(y, sample_off, frame_off, n_takes, max_frames, hop, power, (hipStream_t)stream);
}

int syn_audio_mel_db(const float* y, const int64_t* sample_off, const int64_t* frame_off, int32_t n_takes, int64_t max_frames, int64_t total_frames, double sr,
                     int32_t hop, void* workspace, double* mel_db, void* stream) {
    if (const char* why = audio::bad_batch(y, sample_off, frame_off, n_takes, max_frames, total_frames, hop)) {
        snprintf(g_err, sizeof(g_err), "syn_audio_mel_db: %s", why);
        return -2;
    }
    if (!workspace || !mel_db || ((uintptr_t)workspace & 7)) return fail_msg("syn_audio_mel_db: null pointer, or a workspace that is not 8-byte aligned");
    if (!(sr > 0.0) || !(sr <= 1e9)) return fail_msg("syn_audio_mel_db: the sample rate must be positive");
    if ((total_frames * audio::kMels + 255) / 256 > 0x7fffffffLL) return fail_msg("syn_audio_mel_db: too many frames for one launch");
    hipStream_t s = (hipStream_t)stream;
    if (const int rc = audio::launch_power(y, sample_off, frame_off, n_takes, max_frames, hop, (double*)workspace, s)) return rc;
    audio::MelArgs m = {};
    m.P = (const double*)workspace; m.S = mel_db; m.rows = total_frames; m.df = sr / audio::kNfft;
    audio::mel_edges(sr, m.f);
    hipLaunchKernelGGL(audio::k_mel_db, dim3((unsigned)((total_frames * audio::kMels + 255) / 256)), dim3(256), 0, s, m);
    hipLaunchKernelGGL(audio::k_db_floor, dim3(n_takes), dim3(audio::kWide), 0, s, mel_db, (const long long*)frame_off, 80.0);
    return launched("k_mel_db launches");
}

int syn_audio_onset_env(const double* mel_db, const int64_t* frame_off, int32_t n_takes, int64_t max_frames, int32_t hop, double* env, double* env_norm,
                        void* stream) {
    if (!mel_db || !frame_off || !env || !env_norm) return fail_msg("syn_audio_onset_env: null pointer");
    if (n_takes < 1 || n_takes > 65535) return fail_msg("syn_audio_onset_env: 1 to 65535 takes a call");
    if (max_frames < 1 || (max_frames + audio::kFluxFrames - 1) / audio::kFluxFrames > 0x7fffffffLL) return fail_msg("syn_audio_onset_env: max_frames is the longest take's frames, at least 1");
    if (hop < 1 || hop > audio::kNfft) return fail_msg("syn_audio_onset_env: hop is 1 to 2048");
    const int lag = 1 + audio::kNfft / (2 * hop);                              // the difference's lag plus the centring shift n_fft // (2 hop)
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(audio::k_flux, dim3((unsigned)((max_frames + audio::kFluxFrames - 1) / audio::kFluxFrames), n_takes), dim3(128), 0, s, mel_db,
                       (const long long*)frame_off, lag, env);
    hipLaunchKernelGGL(audio::k_env_norm, dim3(n_takes), dim3(audio::kWide), 0, s, (const long long*)frame_off, (const double*)env, env_norm);
    return launched("k_flux launches");
}

int syn_audio_peak_pick(const double* x, const double* env_raw, const int64_t* frame_off, int32_t n_takes, int32_t pre_max, int32_t post_max, int32_t pre_avg,
                        int32_t post_avg, int32_t wait, double delta, uint8_t* mask, int32_t* count, void* stream) {
    if (!x || !frame_off || !mask || !count) return fail_msg("syn_audio_peak_pick: null pointer");
    if (n_takes < 1 || n_takes > 65535) return fail_msg("syn_audio_peak_pick: 1 to 65535 takes a call");
    if (pre_max < 0 || pre_avg < 0 || wait < 0 || post_max < 1 || post_avg < 1) return fail_msg("syn_audio_peak_pick: pre_max, pre_avg, wait >= 0 and post_max, post_avg >= 1");
    if (!(delta == delta)) return fail_msg("syn_audio_peak_pick: delta is not a number");
    audio::PeakArgs a = {};
    a.x = x; a.raw = env_raw; a.foff = (const long long*)frame_off; a.mask = mask; a.count = count;
    a.pre_max = pre_max; a.post_max = post_max; a.pre_avg = pre_avg; a.post_avg = post_avg; a.wait = wait; a.delta = delta;
    hipLaunchKernelGGL(audio::k_peak_pick, dim3(n_takes), dim3(256), 0, (hipStream_t)stream, a);
    return launched("k_peak_pick launch");
}

}  // extern "C"
