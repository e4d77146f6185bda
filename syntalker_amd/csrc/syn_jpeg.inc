// Baseline JPEG on the device (DESIGN.md 24): the frames syn_render_shade left in device memory become complete JFIF files before they cross to the
// host - what the reference hands to ffmpeg (utils/media.py convert_img_to_mp4) stays on the card until it is 50 times smaller.  The rules are in
// include/syn_hip.h, restated in numpy by tests/jpeg_ref.py; every operation is integer, so the bytes are the restatement's.  Included by syn_kernels.hip.
//
//   k_jpeg_transform  a workgroup takes four MCUs of one MCU row (64 x 16 pixels): each thread reads one 2 x 2 quad (clamped to the image: the padding
//                     repeats the last row and column), makes four Y and one Cb, Cr sample and puts them, level shifted, into the LDS.  Then a wave
//                     owns an MCU: lane (y, u) makes T = (S M^T + 1024) >> 11 of its six blocks, lane (v, u) F = M T, quantises and drops the
//                     int16 at its scan position; the 768 bytes of the MCU leave as three dwords a lane.  No lane idles through either product.
//   k_jpeg_entropy    a wave owns a restart interval (one MCU row) and takes its blocks 64 at a time, a block a lane: the lane codes its block into a
//                     private LDS region of 53 words (a block is at most 20 + 63 * 26 = 1658 bits = 52 words), a wave scan of the bit lengths gives
//                     every block its place, and then every lane builds whole 32-bit words of the interval's stream - it finds the block its word
//                     begins in by bisection and pulls bits from that block's region and the following ones.  Every word has one writer: no atomics.
//                     The bits that do not fill a word are carried into the next round as a segment in front of its blocks.  A second wave scan
//                     over 4 + (0xFF bytes of the word) places the stuffed bytes.  <false> counts the interval's bytes, <true> writes them, by the
//                     same code, at the place k_jpeg_offsets worked out from the counts: count first, write second, no scratch sized by a guess.
//   k_jpeg_offsets    one workgroup: interval sizes -> the first byte of every interval and of every frame (int64), header, RSTn and EOI included.
namespace {
namespace jpeg {

constexpr int kMaxDim = 8192, kMcuBytes = 768, kRegion = 53, kStride = 33;

__device__ const short kM[64] = {
    2896, 2896, 2896, 2896, 2896, 2896, 2896, 2896, 4017, 3406, 2276, 799, -799, -2276, -3406, -4017, 3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784,
    3406, -799, -4017, -2276, 2276, 4017, 799, -3406, 2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896, 2276, -4017, 799, 3406, -3406, -799, 4017, -2276,
    1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567, 799, -2276, 3406, -4017, 4017, -3406, 2276, -799};
__device__ const unsigned char kBase[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
// natural index -> scan position
__device__ const unsigned char kScanPos[64] = {0, 1, 5, 6, 14, 15, 27, 28, 2, 4, 7, 13, 16, 26, 29, 42, 3, 8, 12, 17, 25, 30, 41, 43, 9, 11, 18, 24, 31, 40, 44, 53,
                                               10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

// ---- the Annex K Huffman tables, as (code << 8 | length) per symbol, made from BITS and HUFFVAL at compile time ----
struct Lut { unsigned e[256]; };
struct Spec { unsigned char bits[16]; unsigned char vals[162]; };
constexpr Spec kDcLuma = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr Spec kDcChroma = {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr Spec kAcLuma = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D},
    {1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240, 36, 51, 98, 114, 130, 9, 10, 22, 23,
     24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105,
     106, 115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167,
     168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 225, 226,
     227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250}};
constexpr Spec kAcChroma = {{0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77},
    {0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82, 240, 21, 98, 114, 209, 10, 22, 36, 52, 225,
     37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104,
     105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165,
     166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218,
     226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250}};

constexpr Lut make_lut(const Spec& s) {
    Lut t = {};
    unsigned code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < s.bits[len - 1]; ++i) t.e[s.vals[k++]] = (code++ << 8) | (unsigned)len;
        code <<= 1;
    }
    return t;
}
// [0] DC luminance, [1] DC chrominance, [2] AC luminance, [3] AC chrominance
__device__ const Lut kHuff[4] = {make_lut(kDcLuma), make_lut(kDcChroma), make_lut(kAcLuma), make_lut(kAcChroma)};

__device__ __host__ inline int quant_scale(int quality) { return quality < 50 ? 5000 / quality : 200 - 2 * quality; }

struct Geometry {
    int width, height, mcu_cols, mcu_rows;
};

// ---- colour, subsampling, DCT, quantisation, scan order ----
__global__ __launch_bounds__(256) void k_jpeg_transform(const unsigned char* __restrict__ rgb, long long frame_stride, Geometry g, int groups, int scale,
                                                        unsigned* __restrict__ coef) {
    __shared__ int S[4][6][64];
    __shared__ int T[4][6][64];
    __shared__ __attribute__((aligned(16))) short Z[4][384];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long wg = blockIdx.x;
    const int gx = (int)(wg % groups), my = (int)((wg / groups) % g.mcu_rows);
    const long long f = wg / ((long long)groups * g.mcu_rows);
    {   // a quad a thread: 8 quad rows of 32 quads
        const int qy = tid >> 5, qx = tid & 31, m = qx >> 3;
        if (gx * 4 + m < g.mcu_cols) {
            const unsigned char* img = rgb + f * frame_stride;
            int cb = 0, cr = 0;
#pragma unroll
            for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                for (int dx = 0; dx < 2; ++dx) {
                    const int ly = 2 * qy + dy, lx = 2 * (qx & 7) + dx;                          // inside the MCU
                    const int y = min(my * 16 + ly, g.height - 1), x = min(gx * 64 + m * 16 + lx, g.width - 1);
                    const unsigned char* p = img + ((long long)y * g.width + x) * 3;
                    const int R = p[0], G = p[1], B = p[2];
                    S[m][(ly >> 3) * 2 + (lx >> 3)][(ly & 7) * 8 + (lx & 7)] = ((19595 * R + 38470 * G + 7471 * B + 32768) >> 16) - 128;
                    cb += (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
                    cr += (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
                }
            S[m][4][qy * 8 + (qx & 7)] = ((cb + 2) >> 2) - 128;
            S[m][5][qy * 8 + (qx & 7)] = ((cr + 2) >> 2) - 128;
        }
    }
    __syncthreads();
    const bool live = gx * 4 + wave < g.mcu_cols;                                                // wave-uniform
    const int hi = lane >> 3, u = lane & 7;
    if (live) {                                                                                  // lane (y = hi, u): T[y][u] = (sum_x S[y][x] M[u][x] + 1024) >> 11
        int mu[8];
#pragma unroll
        for (int x = 0; x < 8; ++x) mu[x] = kM[u * 8 + x];
#pragma unroll
        for (int b = 0; b < 6; ++b) {
            int acc = 0;
#pragma unroll
            for (int x = 0; x < 8; ++x) acc += S[wave][b][hi * 8 + x] * mu[x];
            T[wave][b][lane] = (acc + 1024) >> 11;
        }
    }
    __syncthreads();
    if (live) {                                                                                  // lane (v = hi, u): F[v][u] = sum_y M[v][y] T[y][u]
        int mv[8];
#pragma unroll
        for (int y = 0; y < 8; ++y) mv[y] = kM[hi * 8 + y];
        const int pos = kScanPos[lane];
        unsigned q[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) q[c] = (unsigned)min(max(((int)kBase[c][lane] * scale + 50) / 100, 1), 255);
#pragma unroll
        for (int b = 0; b < 6; ++b) {
            int F = 0;
#pragma unroll
            for (int y = 0; y < 8; ++y) F += mv[y] * T[wave][b][y * 8 + u];
            const unsigned Q = q[b >> 2];
            const int mag = (int)(((unsigned)abs(F) + (Q << 14)) / (Q << 15));
            Z[wave][b * 64 + pos] = (short)(F < 0 ? -mag : mag);
        }
    }
    __syncthreads();
    if (live) {
        const long long mcu = (f * g.mcu_rows + my) * g.mcu_cols + gx * 4 + wave;
        const unsigned* z = reinterpret_cast<const unsigned*>(Z[wave]);
#pragma unroll
        for (int k = 0; k < 3; ++k) coef[mcu * (kMcuBytes / 4) + k * 64 + lane] = z[k * 64 + lane];
    }
}

// ---- entropy coding ----
__device__ inline int wave_scan(int v, int lane) {                                               // inclusive, over the 64 lanes
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}

// MSB-first bit writer into a lane's private words
struct Bits {
    unsigned* out;
    unsigned long long acc;
    int n, words;
    __device__ inline void put(unsigned code, int len) {                                         // len <= 27, n < 32 on entry
        acc = (acc << len) | code;
        n += len;
        if (n >= 32) {
            n -= 32;
            out[words++] = (unsigned)(acc >> n);
        }
    }
};

struct EntropyArgs {
    const short* coef;                  // [interval][block][64]
    int* sizes;                         // [interval] entropy bytes, stuffing included (written by <false>, read by <true>)
    const long long* ioff;              // [interval] first entropy byte in data
    const long long* offsets;           // [n_frames + 1]
    const unsigned char* header;
    unsigned char* data;
    long long capacity, n_frames;
    int header_bytes, mcu_cols, mcu_rows;
};

__device__ inline int ff_bytes(unsigned w) {
    return ((w >> 24) == 0xFFu) + (((w >> 16) & 0xFFu) == 0xFFu) + (((w >> 8) & 0xFFu) == 0xFFu) + ((w & 0xFFu) == 0xFFu);
}

template <bool kWrite>
__global__ __launch_bounds__(64) void k_jpeg_entropy(const EntropyArgs a) {
    __shared__ unsigned lut[4][256];
    __shared__ unsigned blk[64 * kStride];              // the round's 64 blocks, 32 dwords each, a dword of padding between them
    __shared__ unsigned region[64 * kRegion];           // a block's code, from bit 0 of its first word
    __shared__ unsigned carry[2][2];                    // the bits a round left over (< 32, from bit 31 down), by the round's parity
    __shared__ int start[66];                           // segment 0: the carry, 1 .. 64: the blocks; start[k]: first bit, start[count + 1]: the total
    const int lane = threadIdx.x;
    const long long interval = blockIdx.x;
    const int row = (int)(interval % a.mcu_rows);
    const long long frame = interval / a.mcu_rows;
    const int n_blocks = a.mcu_cols * 6;
    unsigned char* dst = nullptr;
    int limit = 0;                                      // <true>: the interval's counted bytes; no store goes past them
    if (kWrite) {
        // the counts decide the places; a buffer smaller than their sum is written by nobody, and an interval or a header whose place is not inside
        // the buffer (a workspace that is not syn_jpeg_measure's) is not written either
        if (a.offsets[a.n_frames] > a.capacity) return;
        limit = a.sizes[interval];
        const long long at = a.ioff[interval], head = a.offsets[frame];
        if (limit < 0 || at < 0 || at + limit + 2 > a.capacity || (row == 0 && (head < 0 || head + a.header_bytes > a.capacity))) return;
        dst = a.data + at;
        if (row == 0)
            for (int i = lane; i < a.header_bytes; i += 64) a.data[head + i] = a.header[i];
    }
    for (int i = lane; i < 1024; i += 64) lut[i >> 8][i & 255] = kHuff[i >> 8].e[i & 255];
    if (lane < 4) carry[lane >> 1][lane & 1] = 0;
    const short* src = a.coef + interval * n_blocks * 64;
    const unsigned* src32 = reinterpret_cast<const unsigned*>(src);
    int carry_bits = 0, bytes = 0, parity = 0;
    for (int base = 0; base < n_blocks; base += 64, parity ^= 1) {
        const int count = min(64, n_blocks - base);
        __syncthreads();
        for (int i = lane; i < count * 32; i += 64) blk[(i >> 5) * kStride + (i & 31)] = src32[(long long)base * 32 + i];
        __syncthreads();
        int len = 0;
        if (lane < count) {
            const int gidx = base + lane, b = gidx % 6, mcu = gidx / 6;
            const int prev = b == 0 ? (mcu ? gidx - 3 : -1) : b < 4 ? gidx - 1 : (mcu ? gidx - 6 : -1);  // the component's previous block in the interval
            const unsigned* dc_lut = lut[b < 4 ? 0 : 1];
            const unsigned* ac_lut = lut[b < 4 ? 2 : 3];
            const short* c = reinterpret_cast<const short*>(blk + lane * kStride);
            Bits w = {region + lane * kRegion, 0ull, 0, 0};
            {
                // the transform leaves |DC| <= 1024, |AC| <= 1023; the clamps make the 1658-bit bound hold for any workspace content
                const int d = min(max((int)c[0] - (prev < 0 ? 0 : (int)src[(long long)prev * 64]), -2047), 2047);
                const int size = d ? 32 - __clz(abs(d)) : 0;
                const unsigned e = dc_lut[size];
                w.put(((e >> 8) << size) | (unsigned)((d < 0 ? d - 1 : d) & ((1 << size) - 1)), (int)(e & 255) + size);
            }
            int run = 0;
            for (int k = 1; k < 64; ++k) {
                const int v = min(max((int)c[k], -1023), 1023);
                if (v == 0) { ++run; continue; }
                for (; run >= 16; run -= 16) w.put(ac_lut[0xF0] >> 8, (int)(ac_lut[0xF0] & 255));
                const int size = 32 - __clz(abs(v));
                const unsigned e = ac_lut[(run << 4) | size];
                w.put(((e >> 8) << size) | (unsigned)((v < 0 ? v - 1 : v) & ((1 << size) - 1)), (int)(e & 255) + size);
                run = 0;
            }
            if (run) w.put(ac_lut[0] >> 8, (int)(ac_lut[0] & 255));
            len = w.words * 32 + w.n;
            w.out[w.words] = w.n ? (unsigned)(w.acc << (32 - w.n)) : 0u;
            w.out[w.words + 1] = 0u;                    // a reader takes two words at a time; words <= 51 here, so this stays inside the region
        }
        const int end = wave_scan(len, lane) + carry_bits;
        if (lane == 0) start[0] = 0;
        start[lane + 1] = end - len;
        if (lane == count - 1) start[count + 1] = end;
        __syncthreads();
        const int total = start[count + 1], n_words = total >> 5, left = total & 31;
        // every lane builds words lane, lane + 64, ... of the round's stream; the word behind the last whole one holds the bits that are carried
        for (int w0 = 0; w0 <= n_words; w0 += 64) {
            const int wi = w0 + lane;
            const bool whole = wi < n_words, tail = wi == n_words && left > 0;
            unsigned word = 0;
            if (whole || tail) {
                int pos = wi * 32, need = tail ? left : 32, lo = 0, hi2 = count + 1;
                while (hi2 - lo > 1) {                  // the last segment that starts at or before pos (an empty carry is passed over)
                    const int mid = (lo + hi2) >> 1;
                    if (start[mid] <= pos) lo = mid; else hi2 = mid;
                }
                int seg = lo;
                while (need > 0) {
                    const int off = pos - start[seg], avail = start[seg + 1] - pos, take = min(need, avail);
                    const unsigned* r = seg ? region + (seg - 1) * kRegion : carry[parity];
                    const unsigned long long two = ((unsigned long long)r[off >> 5] << 32) | r[(off >> 5) + 1];
                    const unsigned bits = (unsigned)((two << (off & 31)) >> (64 - take));
                    word |= take == 32 ? bits : bits << (32 - (pos & 31) - take);
                    need -= take;
                    pos += take;
                    seg += take == avail;
                }
            }
            if (tail) { carry[parity ^ 1][0] = word; carry[parity ^ 1][1] = 0; }
            const int mine = whole ? 4 + ff_bytes(word) : 0;
            const int after = wave_scan(mine, lane);
            if (kWrite && whole) {
                int at = bytes + (after - mine);
#pragma unroll
                for (int k = 3; k >= 0; --k) {
                    const unsigned char byte = (unsigned char)(word >> (8 * k));
                    if (at < limit) dst[at] = byte;
                    ++at;
                    if (byte == 0xFF) {
                        if (at < limit) dst[at] = 0;
                        ++at;
                    }
                }
            }
            bytes += __shfl(after, 63, 64);
        }
        carry_bits = left;
    }
    __syncthreads();
    if (lane == 0) {                                    // the interval's last bits, filled with ones to a byte; then its marker
        const unsigned word = carry[parity][0] | (carry_bits ? 0xFFFFFFFFu >> carry_bits : 0u);
        for (int k = 0; k < (carry_bits + 7) / 8; ++k) {
            const unsigned char byte = (unsigned char)(word >> (24 - 8 * k));
            if (kWrite && bytes < limit) dst[bytes] = byte;
            ++bytes;
            if (byte == 0xFF) {
                if (kWrite && bytes < limit) dst[bytes] = 0;
                ++bytes;
            }
        }
        if (kWrite) {
            dst[limit] = 0xFF;
            dst[limit + 1] = row + 1 < a.mcu_rows ? (unsigned char)(0xD0 + (row & 7)) : (unsigned char)0xD9;
        } else {
            a.sizes[interval] = bytes;
        }
    }
}

// interval i of frame f, row r occupies [header of the frame if r = 0][sizes[i] entropy bytes][2 marker bytes]
__global__ __launch_bounds__(256) void k_jpeg_offsets(const int* __restrict__ sizes, long long n_frames, int mcu_rows, int header_bytes,
                                                      long long* __restrict__ ioff, long long* __restrict__ offsets) {
    __shared__ long long part[256];
    const int tid = threadIdx.x;
    const long long n = n_frames * mcu_rows, per = (n + 255) / 256, lo = min(n, tid * per), hi = min(n, lo + per);
    long long sum = 0;
    for (long long i = lo; i < hi; ++i) sum += sizes[i] + 2 + (i % mcu_rows == 0 ? header_bytes : 0);
    part[tid] = sum;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const long long o = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += o;
        __syncthreads();
    }
    long long at = part[tid] - sum;
    for (long long i = lo; i < hi; ++i) {
        const bool first = i % mcu_rows == 0;
        if (first) offsets[i / mcu_rows] = at;
        ioff[i] = at + (first ? header_bytes : 0);
        at += sizes[i] + 2 + (first ? header_bytes : 0);
    }
    if (tid == 255) offsets[n_frames] = part[255];
}

struct Plan {
    Geometry g;
    long long intervals, coef_bytes, sizes_at, ioff_at, total;
};

// nullptr, or why the call cannot run
static const char* plan(int64_t n_frames, int32_t width, int32_t height, Plan* p) {
    if (width < 1 || width > kMaxDim || height < 1 || height > kMaxDim) return "width and height are 1 to 8192 pixels";
    if (n_frames < 0) return "negative frame count";
    p->g = {width, height, (width + 15) / 16, (height + 15) / 16};
    p->intervals = n_frames * p->g.mcu_rows;
    if (n_frames > (1LL << 31) || p->intervals * ((p->g.mcu_cols + 3) / 4) > 0x7fffffffLL) return "too many frames for one launch";
    p->coef_bytes = p->intervals * p->g.mcu_cols * kMcuBytes;
    p->sizes_at = p->coef_bytes;
    p->ioff_at = (p->sizes_at + p->intervals * 4 + 15) / 16 * 16;
    p->total = p->ioff_at + p->intervals * 8;
    return nullptr;
}

}  // namespace jpeg
}  // namespace

// ---- entry points -----------------------------------------------------------------------------------------------------------------------------------
extern "C" {

int64_t syn_jpeg_workspace_bytes(int64_t n_frames, int32_t width, int32_t height) {
    jpeg::Plan p;
    if (n_frames < 1 || jpeg::plan(n_frames, width, height, &p)) return -1;
    return p.total;
}

int syn_jpeg_transform(const uint8_t* rgb, int64_t frame_stride, int64_t n_frames, int32_t width, int32_t height, int32_t quality, void* workspace,
                       void* stream) {
    jpeg::Plan p;
    if (const char* why = jpeg::plan(n_frames, width, height, &p)) {
        snprintf(g_err, sizeof(g_err), "syn_jpeg_transform: %s", why);
        return -2;
    }
    if (quality < 1 || quality > 100) return fail_msg("syn_jpeg_transform: quality is 1 to 100");
    if (frame_stride < (int64_t)width * height * 3) return fail_msg("syn_jpeg_transform: frame_stride is at least width * height * 3 bytes");
    if (n_frames == 0) return 0;
    if (!rgb || !workspace) return fail_msg("syn_jpeg_transform: null pointer");
    if ((uintptr_t)workspace & 15) return fail_msg("syn_jpeg_transform: the workspace must be 16-byte aligned");
    const int groups = (p.g.mcu_cols + 3) / 4;
    hipLaunchKernelGGL(jpeg::k_jpeg_transform, dim3((unsigned)(p.intervals * groups)), dim3(256), 0, (hipStream_t)stream, rgb, (long long)frame_stride, p.g, groups,
                       jpeg::quant_scale(quality), (unsigned*)workspace);
    return launched("k_jpeg_transform launch");
}

int syn_jpeg_measure(int64_t n_frames, int32_t width, int32_t height, int32_t header_bytes, void* workspace, int64_t* offsets, void* stream) {
    jpeg::Plan p;
    if (const char* why = jpeg::plan(n_frames, width, height, &p)) {
        snprintf(g_err, sizeof(g_err), "syn_jpeg_measure: %s", why);
        return -2;
    }
    if (header_bytes < 0 || header_bytes > 65536) return fail_msg("syn_jpeg_measure: header_bytes is 0 to 65536");
    if (n_frames == 0) return 0;
    if (!workspace || !offsets) return fail_msg("syn_jpeg_measure: null pointer");
    if ((uintptr_t)workspace & 15) return fail_msg("syn_jpeg_measure: the workspace must be 16-byte aligned");
    char* ws = (char*)workspace;
    jpeg::EntropyArgs a = {};
    a.coef = (const short*)ws; a.sizes = (int*)(ws + p.sizes_at); a.mcu_cols = p.g.mcu_cols; a.mcu_rows = p.g.mcu_rows; a.n_frames = n_frames;
    hipLaunchKernelGGL(jpeg::k_jpeg_entropy<false>, dim3((unsigned)p.intervals), dim3(64), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(jpeg::k_jpeg_offsets, dim3(1), dim3(256), 0, (hipStream_t)stream, (const int*)a.sizes, (long long)n_frames, p.g.mcu_rows, (int)header_bytes,
                       (long long*)(ws + p.ioff_at), (long long*)offsets);
    return launched("k_jpeg_entropy<count> / k_jpeg_offsets launches");
}

int syn_jpeg_write(int64_t n_frames, int32_t width, int32_t height, const uint8_t* header, int32_t header_bytes, const void* workspace, const int64_t* offsets,
                   uint8_t* data, int64_t capacity, void* stream) {
    jpeg::Plan p;
    if (const char* why = jpeg::plan(n_frames, width, height, &p)) {
        snprintf(g_err, sizeof(g_err), "syn_jpeg_write: %s", why);
        return -2;
    }
    if (header_bytes < 0 || header_bytes > 65536) return fail_msg("syn_jpeg_write: header_bytes is 0 to 65536");
    if (capacity < 0) return fail_msg("syn_jpeg_write: negative capacity");
    if (n_frames == 0) return 0;
    if (!workspace || !offsets || !data || (header_bytes && !header)) return fail_msg("syn_jpeg_write: null pointer");
    if ((uintptr_t)workspace & 15) return fail_msg("syn_jpeg_write: the workspace must be 16-byte aligned");
    const char* ws = (const char*)workspace;
    jpeg::EntropyArgs a = {};
    a.coef = (const short*)ws; a.sizes = (int*)(ws + p.sizes_at); a.ioff = (const long long*)(ws + p.ioff_at); a.offsets = (const long long*)offsets;
    a.header = header; a.data = data; a.capacity = capacity; a.n_frames = n_frames; a.header_bytes = header_bytes; a.mcu_cols = p.g.mcu_cols; a.mcu_rows = p.g.mcu_rows;
    hipLaunchKernelGGL(jpeg::k_jpeg_entropy<true>, dim3((unsigned)p.intervals), dim3(64), 0, (hipStream_t)stream, a);
    return launched("k_jpeg_entropy<write> launch");
}

}  // extern "C"
