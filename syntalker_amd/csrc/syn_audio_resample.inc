// Audio resampling (DESIGN.md 25): a waveform at any integer rate to any other, what the reference takes from librosa.load + librosa.resample
// (dataloaders/beat_sep_lower.py:392-393, diffusion_rvqvae_trainer.py:679-680, demo.py:64).  Band-limited interpolation with a Kaiser-windowed sinc
// (64 zero crossings a side, the design resampy publishes as kaiser_best), evaluated exactly on the rational grid: for up / down = L / M in lowest terms
//
//   y[m] = sum_j x[j] h[m M - j L],   m = 0 .. ceil(n L / M) - 1,   x zero outside 0 .. n - 1,   h[k] = 0 for |k| > K.
//
// With m M = j0 L + p (0 <= p < L) the term of sample j has k = p + (j0 - j) L, and |k| <= K leaves j0 - W <= j <= j0 + W + 1, W = K / L: at most
// T = 2 W + 2 samples, the same count for every phase.  The phase of output m depends on r = m mod L alone, p = (r M) mod L, and consecutive outputs
// have consecutive r: the host packs the taps in PAIRS, TAP-MAJOR over r, taps[t / 2][r][t % 2] = h[p(r) + (W - t) L] (zero where |k| > K),
// t = 0 .. T - 1, so that the thread of output m walks column r of the table downwards, 16 bytes a step, while it walks x[j0 - W + t] upwards, and a
// wave's 64 threads read 1 KB of contiguous table at every step.
//
//   k_resample   a workgroup of 256 threads owns 256 consecutive outputs of one take, a thread one output.  The workgroup's samples - from the first
//                output's j0 - W to the last one's j0 + W + 1 - pass through the LDS as fp32 in chunks of 2048 (one chunk at 22.05, 44.1 and 48 kHz
//                to 16 kHz; a ratio with a long filter or a large M / L takes several).  The span is cut to the take, 0 .. n - 1, before anything is
//                staged: a sample outside the take is a zero term, left out, and no thread reads another take's samples.  Within a chunk a thread adds
//                its terms in ASCENDING j, acc = fma((double)x[j], tap, acc), one chain from acc = 0: the chunking does not change the order, and
//                fma(0, h, acc) = acc for the terms left out.  The sum is written as it is (out64) and rounded once to fp32 (out32).  Taps are read
//                two at a time, with a lone tap in front of or behind the pairs where a chunk or the take's end cuts a column at an odd t.
//                Every index that scales with the take - m M, the sample and output offsets - is 64-bit.
namespace {
namespace audio {

constexpr int kRsThreads = 256, kRsChunk = 2048;
typedef double d2 __attribute__((ext_vector_type(2)));

struct ResampleArgs {
    const float* y; const long long* soff; const long long* ooff;
    const double* taps;              // [T / 2][L][2]
    float* out32; double* out64;
    long long L, M;
    int T;                           // 2 W + 2
};

__global__ __launch_bounds__(kRsThreads) void k_resample(const ResampleArgs a) {
    __shared__ __attribute__((aligned(16))) float win[kRsChunk];
    const int tid = threadIdx.x;
    const long long s0 = a.soff[blockIdx.y], n = a.soff[blockIdx.y + 1] - s0;
    const long long n_out = (n * a.L + a.M - 1) / a.M;
    const long long m0 = (long long)blockIdx.x * kRsThreads;
    if (m0 >= n_out) return;                                                   // the whole workgroup: nothing waits at a barrier
    const long long m_last = m0 + kRsThreads - 1 < n_out ? m0 + kRsThreads - 1 : n_out - 1;
    const int W = a.T / 2 - 1;
    // the workgroup's samples, cut to the take
    long long lo = m0 * a.M / a.L - W, hi = m_last * a.M / a.L + W + 1;
    lo = lo < 0 ? 0 : lo;
    hi = hi > n - 1 ? n - 1 : hi;
    // this thread's output: samples ja .. ja + T - 1 against column r, cut to the take
    const long long m = m0 + tid;
    const bool live = m < n_out;
    const long long mm = live ? m * a.M : 0, j0 = mm / a.L, ja = j0 - W, r = live ? m % a.L : 0;
    long long jb = live ? ja + a.T - 1 : ja - 1;                               // a thread past the take's end has no terms
    jb = jb > n - 1 ? n - 1 : jb;
    const double* __restrict__ col = a.taps + 2 * r;                            // tap t of this column: col[(t / 2) 2 L + t % 2]
    double acc = 0.0;
    for (long long cs = lo; cs <= hi; cs += kRsChunk) {
        const int cn = hi - cs + 1 < kRsChunk ? (int)(hi - cs + 1) : kRsChunk;  // 0 <= cs, cs + cn - 1 <= hi <= n - 1: inside the take
        for (int i = tid; i < cn; i += kRsThreads) win[i] = a.y[s0 + cs + i];
        __syncthreads();
        const long long ce = cs + kRsChunk - 1;
        long long b = ja > cs ? ja : cs, e = jb < ce ? jb : ce;               // this thread's samples in the chunk: b .. e, ascending
        if (b <= e) {
            int t = (int)(b - ja), x = (int)(b - cs);
            const int t_end = (int)(e - ja);                                   // inclusive
            const long long pitch = 2 * a.L;
            if (t & 1) { acc = __builtin_fma((double)win[x], col[(t >> 1) * pitch + 1], acc); ++t; ++x; }
            const double* q = col + (t >> 1) * pitch;
#pragma unroll 4
            for (; t + 1 <= t_end; t += 2, x += 2, q += pitch) {               // unrolled for loads in flight; the chain's order is the loop's
                const d2 h = *reinterpret_cast<const d2*>(q);
                acc = __builtin_fma((double)win[x], h.x, acc);
                acc = __builtin_fma((double)win[x + 1], h.y, acc);
            }
            if (t == t_end) acc = __builtin_fma((double)win[x], q[0], acc);
        }
        __syncthreads();
    }
    if (live) {
        const long long o = a.ooff[blockIdx.y] + m;
        if (a.out64) a.out64[o] = acc;
        if (a.out32) a.out32[o] = (float)acc;
    }
}

static long long gcd_ll(long long x, long long y) {
    while (y) { const long long t = x % y; x = y; y = t; }
    return x;
}

}  // namespace audio
}  // namespace

extern "C" {

int syn_audio_resample(const float* y, const int64_t* sample_off, const int64_t* out_off, int32_t n_takes, int64_t max_samples, int32_t up, int32_t down,
                       const double* taps, int64_t n_taps, float* out32, double* out64, void* stream) {
    if (!y || !sample_off || !out_off || !taps) return fail_msg("syn_audio_resample: null pointer");
    if (!out32 && !out64) return fail_msg("syn_audio_resample: null pointer (out32 and out64 are both NULL)");
    if (n_takes < 1 || n_takes > 65535) return fail_msg("syn_audio_resample: 1 to 65535 takes a call");
    if (up < 1 || down < 1) return fail_msg("syn_audio_resample: up and down are at least 1");
    if (audio::gcd_ll(up, down) != 1) return fail_msg("syn_audio_resample: up and down must be coprime (gcd(up, down) = 1)");
    if (n_taps < 0) return fail_msg("syn_audio_resample: a negative table size");
    if (n_taps < 2LL * up || n_taps % (2LL * up) || n_taps / up > 0x7ffffffeLL) return fail_msg("syn_audio_resample: the table size is a whole number of pair rows, at least 1, of 2 up taps");
    if (((uintptr_t)taps & 15) || ((uintptr_t)out64 & 7)) return fail_msg("syn_audio_resample: misaligned fp64 pointer (taps: 16 bytes, out64: 8)");
    if (max_samples < 1 || max_samples > (1LL << 46) / up) return fail_msg("syn_audio_resample: max_samples is the longest take's samples, 1 .. 2^46 / up");
    const int64_t max_out = (max_samples * up + down - 1) / down, blocks = (max_out + audio::kRsThreads - 1) / audio::kRsThreads;
    if (blocks > 0x7fffffffLL) return fail_msg("syn_audio_resample: too many samples in a take for one launch");
    audio::ResampleArgs a = {};
    a.y = y; a.soff = (const long long*)sample_off; a.ooff = (const long long*)out_off; a.taps = taps; a.out32 = out32; a.out64 = out64;
    a.L = up; a.M = down; a.T = (int)(n_taps / up);
    hipLaunchKernelGGL(audio::k_resample, dim3((unsigned)blocks, n_takes), dim3(audio::kRsThreads), 0, (hipStream_t)stream, a);
    return launched("k_resample launch");
}

}  // extern "C"
