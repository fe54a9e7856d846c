// ugs_wl.hip -- Weisfeiler-Lehman graph hashes and vocabulary ids of sampled subgraphs, on the device.
// Replaces the host loop of the reference's SS-GNN-WL consumer (src/gps/gps/models/ss_gnn_wl.py:210-247 with
// src/gps/gps/utils/wl_vocab.py:21-67): per sample one networkx.weisfeiler_lehman_graph_hash(G, node_attr='attr', iterations)
// with the degree as attribute -- or, with node features, the first 8 hex characters of the md5 of the vertex's feature row -- and
// a dict lookup.  The law is stated at ugs_wl_hash and ugs_wl_hash_labeled in include/ugs_mi355.h; the digests are networkx
// 3.4.2's, bit for bit.
//
// ugs_wl_feature_labels_kernel: one lane per feature row, MD5 (RFC 1321) of its bytes; the label is the digest's first four bytes.
// ugs_wl_hash_kernel: one lane group (8, 16 or 32 lanes, by k) per sample, one lane per vertex; groups never span a wave.
//   edges   the group's lanes stride over the row's edge entries and OR them into one 32-bit neighbour mask per vertex in LDS:
//           range check, deduplication, reversed copies and loops at once;
//   labels  128-bit, two uint64 compared big-endian, double-buffered in LDS.  The start labels are the degrees' decimal strings
//           packed into the top bytes of the high word, so that the same comparison gives Python's string order ("10" < "2").
//           Label mode (a launch argument, the same code): the j-th valid slot of the row is vertex j (prefix popcount of the
//           group's ballot) and puts labels[id] into the top 32 bits of the high word; its first message takes it as one piece of
//           8 hex characters; an id or label out of range raises the group's flag: status 3;
//   order   once per iteration every lane ranks its label among the group's (ties by vertex): order[rank] = vertex.  A vertex
//           walks that list and keeps its neighbours -- its sorted neighbour labels -- and the run heads of the same list are the
//           iteration's Counter items;
//   BLAKE2b a message is produced in pieces of at most 8 bytes (a decimal label, 8 hex characters, punctuation) that are shifted
//           into 64-bit words and stored into the lane's 128-byte staging block in LDS; a full block is read back as sixteen
//           whole words and compressed only once more data arrives or the message ends, so a message of exactly 128 or 256
//           bytes ends with its full block and the final flag.  The twelve rounds are written out with the sigma schedule as
//           literals: m[16] and v[16] stay in registers (0 bytes of scratch);
//   final   lane 0 of the group streams str(tuple(items)) through the same piece routine, its state kept across iterations.
// ugs_wl_lookup_kernel: one lane per row, binary search of the digest in the sorted key table.
#include "ugs_device.h"
#include "../../include/ugs_mi355.h"

#define UGS_WL_MAX_ITER 8
#define UGS_WL_BLOCK 256

namespace {

typedef unsigned long long u64;

#define WL_IV0 0x6a09e667f3bcc908ull
#define WL_IV1 0xbb67ae8584caa73bull
#define WL_IV2 0x3c6ef372fe94f82bull
#define WL_IV3 0xa54ff53a5f1d36f1ull
#define WL_IV4 0x510e527fade682d1ull
#define WL_IV5 0x9b05688c2b3e6c1full
#define WL_IV6 0x1f83d9abfb41bd6bull
#define WL_IV7 0x5be0cd19137e2179ull

__device__ __forceinline__ u64 rotr64(u64 x, int r) { return (x >> r) | (x << (64 - r)); }

#define WL_G(a, b, c, d, x, y) \
    a = a + b + (x); d = rotr64(d ^ a, 32); c = c + d; b = rotr64(b ^ c, 24); \
    a = a + b + (y); d = rotr64(d ^ a, 16); c = c + d; b = rotr64(b ^ c, 63);
#define WL_ROUND(s0, s1, s2, s3, s4, s5, s6, s7, s8, s9, s10, s11, s12, s13, s14, s15) \
    WL_G(v0, v4, v8, v12, m[s0], m[s1]) WL_G(v1, v5, v9, v13, m[s2], m[s3]) WL_G(v2, v6, v10, v14, m[s4], m[s5]) WL_G(v3, v7, v11, v15, m[s6], m[s7]) \
    WL_G(v0, v5, v10, v15, m[s8], m[s9]) WL_G(v1, v6, v11, v12, m[s10], m[s11]) WL_G(v2, v7, v8, v13, m[s12], m[s13]) WL_G(v3, v4, v9, v14, m[s14], m[s15])

// BLAKE2b compression function F (RFC 7693 section 3.2): t = bytes of the message up to and including this block
__device__ __forceinline__ void blake2b_compress(u64 (&h)[8], const u64 (&m)[16], u64 t, bool last) {
    u64 v0 = h[0], v1 = h[1], v2 = h[2], v3 = h[3], v4 = h[4], v5 = h[5], v6 = h[6], v7 = h[7];
    u64 v8 = WL_IV0, v9 = WL_IV1, v10 = WL_IV2, v11 = WL_IV3, v12 = WL_IV4 ^ t, v13 = WL_IV5, v14 = last ? ~WL_IV6 : WL_IV6, v15 = WL_IV7;
    WL_ROUND(0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)
    WL_ROUND(14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3)
    WL_ROUND(11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4)
    WL_ROUND(7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8)
    WL_ROUND(9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13)
    WL_ROUND(2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9)
    WL_ROUND(12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11)
    WL_ROUND(13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10)
    WL_ROUND(6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5)
    WL_ROUND(10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0)
    WL_ROUND(0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)
    WL_ROUND(14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3)
    h[0] ^= v0 ^ v8; h[1] ^= v1 ^ v9; h[2] ^= v2 ^ v10; h[3] ^= v3 ^ v11;
    h[4] ^= v4 ^ v12; h[5] ^= v5 ^ v13; h[6] ^= v6 ^ v14; h[7] ^= v7 ^ v15;
}

// one unkeyed BLAKE2b-128 stream: chaining value, the word being assembled, bytes taken so far
struct WlStream {
    u64 h[8];
    u64 acc;
    unsigned pos;
};

__device__ __forceinline__ void wl_stream_init(WlStream &s) {
    s.h[0] = WL_IV0 ^ 0x01010010ull;      // parameter block: digest_length 16, no key, fanout 1, depth 1
    s.h[1] = WL_IV1; s.h[2] = WL_IV2; s.h[3] = WL_IV3; s.h[4] = WL_IV4; s.h[5] = WL_IV5; s.h[6] = WL_IV6; s.h[7] = WL_IV7;
    s.acc = 0;
    s.pos = 0;
}

enum { WL_PIECE = 0, WL_FLUSH = 1, WL_FINISH = 2 };

// One step of a stream.  WL_PIECE appends the low n bytes of v (1 <= n <= 8, first byte lowest, the bytes above n zero); WL_FLUSH
// stores a started word; WL_FINISH pads the block with zero words and compresses it with the final flag.  A full block waits in
// the staging words stg[j * ld], j = 0..15, until the next word is about to overwrite word 0, so the block that ends the message
// is always the one compressed by WL_FINISH -- also when the message is an exact multiple of 128 bytes.  The compression
// function appears once per call site of this routine.
__device__ __forceinline__ void wl_stream_step(WlStream &s, u64 *stg, int ld, int what, u64 v, unsigned n) {
    const unsigned off = s.pos & 7u;
    const unsigned widx = (s.pos >> 3) & 15u;
    bool store = false;
    u64 word = s.acc;
    if (what == WL_PIECE) {
        word |= v << (8u * off);
        store = off + n >= 8u;
    } else if (what == WL_FLUSH) {
        store = off != 0u;
    } else {
        const unsigned used = s.pos ? (((s.pos - 1u) & 127u) >> 3) + 1u : 0u;      // words of the last block that hold message bytes
        for (unsigned j = used; j < 16u; ++j) stg[j * ld] = 0;
    }
    if (what == WL_FINISH || (store && widx == 0u && s.pos >= 128u)) {
        u64 m[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) m[j] = stg[j * ld];
        blake2b_compress(s.h, m, what == WL_FINISH ? (u64)s.pos : (u64)(s.pos & ~127u), what == WL_FINISH);
    }
    if (store) {
        stg[widx * ld] = word;
        s.acc = (what == WL_PIECE && off != 0u) ? v >> (8u * (8u - off)) : 0;
    } else {
        s.acc = word;
    }
    if (what == WL_PIECE) s.pos += n;
}

// the 32 bits of x as 8 lowercase hex characters, most significant nibble in the lowest byte
__device__ __forceinline__ u64 hex8(unsigned x) {
    u64 t = x;
    t = ((t & 0xffff0000ull) << 16) | (t & 0xffffull);
    t = ((t & 0x0000ff000000ff00ull) << 8) | (t & 0x000000ff000000ffull);
    t = ((t & 0x00f000f000f000f0ull) << 4) | (t & 0x000f000f000f000full);      // byte j = nibble j, least significant first
    t = __builtin_bswap64(t);
    const u64 gt9 = ((t + 0x0606060606060606ull) >> 4) & 0x0101010101010101ull;
    return t + 0x3030303030303030ull + gt9 * 39ull;
}

// a count or degree of at most 99 as its decimal characters, first one lowest; *len = 1 or 2
__device__ __forceinline__ u64 dec2(unsigned d, unsigned *len) {
    if (d < 10u) { *len = 1; return (u64)('0' + d); }
    *len = 2;
    return (u64)('0' + d / 10u) | ((u64)('0' + d % 10u) << 8);
}

__device__ __forceinline__ unsigned hex_word(u64 hi, u64 lo, int p) {      // 32-bit quarter p = 0..3 of the label, most significant first
    const u64 w = p < 2 ? hi : lo;
    return (unsigned)((p & 1) ? w : (w >> 32));
}

// ---- MD5 (RFC 1321) of feature rows: the start labels of the node-feature form ----
__device__ __forceinline__ unsigned rotl32(unsigned x, int r) { return (x << r) | (x >> (32 - r)); }

#define MD5_F(b, c, d) ((d) ^ ((b) & ((c) ^ (d))))
#define MD5_G(b, c, d) ((c) ^ ((d) & ((b) ^ (c))))
#define MD5_H(b, c, d) ((b) ^ (c) ^ (d))
#define MD5_I(b, c, d) ((c) ^ ((b) | ~(d)))
#define MD5_STEP(f, a, b, c, d, x, t, s) a += f(b, c, d) + (x) + (t); a = rotl32(a, s) + b;

// one 64-byte block, m[j] = its bytes 4j .. 4j+3 little-endian; the four rounds written out with the constants as literals
__device__ __forceinline__ void md5_block(unsigned (&h)[4], const unsigned (&m)[16]) {
    unsigned a = h[0], b = h[1], c = h[2], d = h[3];
    MD5_STEP(MD5_F, a, b, c, d, m[0], 0xd76aa478u, 7) MD5_STEP(MD5_F, d, a, b, c, m[1], 0xe8c7b756u, 12)
    MD5_STEP(MD5_F, c, d, a, b, m[2], 0x242070dbu, 17) MD5_STEP(MD5_F, b, c, d, a, m[3], 0xc1bdceeeu, 22)
    MD5_STEP(MD5_F, a, b, c, d, m[4], 0xf57c0fafu, 7) MD5_STEP(MD5_F, d, a, b, c, m[5], 0x4787c62au, 12)
    MD5_STEP(MD5_F, c, d, a, b, m[6], 0xa8304613u, 17) MD5_STEP(MD5_F, b, c, d, a, m[7], 0xfd469501u, 22)
    MD5_STEP(MD5_F, a, b, c, d, m[8], 0x698098d8u, 7) MD5_STEP(MD5_F, d, a, b, c, m[9], 0x8b44f7afu, 12)
    MD5_STEP(MD5_F, c, d, a, b, m[10], 0xffff5bb1u, 17) MD5_STEP(MD5_F, b, c, d, a, m[11], 0x895cd7beu, 22)
    MD5_STEP(MD5_F, a, b, c, d, m[12], 0x6b901122u, 7) MD5_STEP(MD5_F, d, a, b, c, m[13], 0xfd987193u, 12)
    MD5_STEP(MD5_F, c, d, a, b, m[14], 0xa679438eu, 17) MD5_STEP(MD5_F, b, c, d, a, m[15], 0x49b40821u, 22)
    MD5_STEP(MD5_G, a, b, c, d, m[1], 0xf61e2562u, 5) MD5_STEP(MD5_G, d, a, b, c, m[6], 0xc040b340u, 9)
    MD5_STEP(MD5_G, c, d, a, b, m[11], 0x265e5a51u, 14) MD5_STEP(MD5_G, b, c, d, a, m[0], 0xe9b6c7aau, 20)
    MD5_STEP(MD5_G, a, b, c, d, m[5], 0xd62f105du, 5) MD5_STEP(MD5_G, d, a, b, c, m[10], 0x02441453u, 9)
    MD5_STEP(MD5_G, c, d, a, b, m[15], 0xd8a1e681u, 14) MD5_STEP(MD5_G, b, c, d, a, m[4], 0xe7d3fbc8u, 20)
    MD5_STEP(MD5_G, a, b, c, d, m[9], 0x21e1cde6u, 5) MD5_STEP(MD5_G, d, a, b, c, m[14], 0xc33707d6u, 9)
    MD5_STEP(MD5_G, c, d, a, b, m[3], 0xf4d50d87u, 14) MD5_STEP(MD5_G, b, c, d, a, m[8], 0x455a14edu, 20)
    MD5_STEP(MD5_G, a, b, c, d, m[13], 0xa9e3e905u, 5) MD5_STEP(MD5_G, d, a, b, c, m[2], 0xfcefa3f8u, 9)
    MD5_STEP(MD5_G, c, d, a, b, m[7], 0x676f02d9u, 14) MD5_STEP(MD5_G, b, c, d, a, m[12], 0x8d2a4c8au, 20)
    MD5_STEP(MD5_H, a, b, c, d, m[5], 0xfffa3942u, 4) MD5_STEP(MD5_H, d, a, b, c, m[8], 0x8771f681u, 11)
    MD5_STEP(MD5_H, c, d, a, b, m[11], 0x6d9d6122u, 16) MD5_STEP(MD5_H, b, c, d, a, m[14], 0xfde5380cu, 23)
    MD5_STEP(MD5_H, a, b, c, d, m[1], 0xa4beea44u, 4) MD5_STEP(MD5_H, d, a, b, c, m[4], 0x4bdecfa9u, 11)
    MD5_STEP(MD5_H, c, d, a, b, m[7], 0xf6bb4b60u, 16) MD5_STEP(MD5_H, b, c, d, a, m[10], 0xbebfbc70u, 23)
    MD5_STEP(MD5_H, a, b, c, d, m[13], 0x289b7ec6u, 4) MD5_STEP(MD5_H, d, a, b, c, m[0], 0xeaa127fau, 11)
    MD5_STEP(MD5_H, c, d, a, b, m[3], 0xd4ef3085u, 16) MD5_STEP(MD5_H, b, c, d, a, m[6], 0x04881d05u, 23)
    MD5_STEP(MD5_H, a, b, c, d, m[9], 0xd9d4d039u, 4) MD5_STEP(MD5_H, d, a, b, c, m[12], 0xe6db99e5u, 11)
    MD5_STEP(MD5_H, c, d, a, b, m[15], 0x1fa27cf8u, 16) MD5_STEP(MD5_H, b, c, d, a, m[2], 0xc4ac5665u, 23)
    MD5_STEP(MD5_I, a, b, c, d, m[0], 0xf4292244u, 6) MD5_STEP(MD5_I, d, a, b, c, m[7], 0x432aff97u, 10)
    MD5_STEP(MD5_I, c, d, a, b, m[14], 0xab9423a7u, 15) MD5_STEP(MD5_I, b, c, d, a, m[5], 0xfc93a039u, 21)
    MD5_STEP(MD5_I, a, b, c, d, m[12], 0x655b59c3u, 6) MD5_STEP(MD5_I, d, a, b, c, m[3], 0x8f0ccc92u, 10)
    MD5_STEP(MD5_I, c, d, a, b, m[10], 0xffeff47du, 15) MD5_STEP(MD5_I, b, c, d, a, m[1], 0x85845dd1u, 21)
    MD5_STEP(MD5_I, a, b, c, d, m[8], 0x6fa87e4fu, 6) MD5_STEP(MD5_I, d, a, b, c, m[15], 0xfe2ce6e0u, 10)
    MD5_STEP(MD5_I, c, d, a, b, m[6], 0xa3014314u, 15) MD5_STEP(MD5_I, b, c, d, a, m[13], 0x4e0811a1u, 21)
    MD5_STEP(MD5_I, a, b, c, d, m[4], 0xf7537e82u, 6) MD5_STEP(MD5_I, d, a, b, c, m[11], 0xbd3af235u, 10)
    MD5_STEP(MD5_I, c, d, a, b, m[2], 0x2ad7d2bbu, 15) MD5_STEP(MD5_I, b, c, d, a, m[9], 0xeb86d391u, 21)
    h[0] += a; h[1] += b; h[2] += c; h[3] += d;
}

struct WlLabelArgs {
    const unsigned char *x;      // row i at x + i * stride, `len` bytes
    int64_t stride, rows;
    unsigned len;                // < 2^29: the bit length fits 32 bits
    int64_t *labels;             // [rows]
};

// One lane per row.  A row that starts on a 4-byte boundary is read in whole words, any other one byte by byte; the last partial
// word, the 0x80 byte, the zero padding and the bit length are put together per word, so m[16] keeps static indices (0 bytes of
// scratch) and nothing past the row's last byte is read.
__global__ __launch_bounds__(256) void ugs_wl_feature_labels_kernel(WlLabelArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.rows) return;
    const unsigned char *p = a.x + i * a.stride;
    const bool aligned = (reinterpret_cast<uintptr_t>(p) & 3u) == 0u;
    const unsigned len = a.len;
    const unsigned nblk = (len + 72u) >> 6;                // len + 0x80 + 8 length bytes, rounded up to blocks
    unsigned h[4] = {0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u};
    for (unsigned blk = 0; blk < nblk; ++blk) {
        unsigned m[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const unsigned o = (blk << 6) + 4u * j;
            unsigned w = 0;
            if (o + 4u <= len) {
                if (aligned) w = *reinterpret_cast<const unsigned *>(p + o);
                else w = (unsigned)p[o] | ((unsigned)p[o + 1] << 8) | ((unsigned)p[o + 2] << 16) | ((unsigned)p[o + 3] << 24);
            } else if (o <= len) {                         // the row's last bytes and the 0x80 behind them
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const unsigned at = o + q;
                    const unsigned byte = at < len ? (unsigned)p[at] : at == len ? 0x80u : 0u;
                    w |= byte << (8 * q);
                }
            }
            m[j] = w;
        }
        if (blk == nblk - 1u) m[14] = len << 3;            // bit length, low word; the high word stays zero
        md5_block(h, m);
    }
    a.labels[i] = (int64_t)__builtin_bswap32(h[0]);        // digest bytes 0-3 as a big-endian number: int(hexdigest()[:8], 16)
}

struct WlHashArgs {
    const int64_t *nodes;        // [rows, k]
    const int64_t *edge_index;   // [2, num_cols], row stride `stride`
    int64_t stride, num_cols;
    const int64_t *edge_ptr;     // [rows + 1]
    int64_t rows;
    int k, iterations, wshift;   // lanes per group = 1 << wshift
    u64 *digest;                 // [rows, 2]
    int32_t *status;             // [rows]
    const int64_t *labels;       // [num_labels]: start labels by vertex id (label mode), values in [0, 2^32)
    int64_t num_labels;
    int labeled;                 // 0: the start labels are the degrees; 1: labels[nodes[row, slot]]
};

__global__ __launch_bounds__(UGS_WL_BLOCK) void ugs_wl_hash_kernel(WlHashArgs a) {
    __shared__ u64 stg_sh[16 * UGS_WL_BLOCK];          // word j of thread t at [j * 256 + t]: a wave's word accesses touch consecutive addresses
    __shared__ u64 fstg_sh[16 * (UGS_WL_BLOCK / 8)];   // staging block of a group's final string: word j of group g at [j * 32 + g]
    __shared__ u64 lab_sh[2][UGS_WL_BLOCK][2];
    __shared__ unsigned mask_sh[UGS_WL_BLOCK];
    __shared__ int bad_sh[UGS_WL_BLOCK / 8];
    __shared__ unsigned char order_sh[UGS_WL_BLOCK], cnt_sh[UGS_WL_BLOCK];

    const int tid = (int)threadIdx.x;
    const int W = 1 << a.wshift;
    const int g = tid >> a.wshift;                     // group inside the block
    const int u = tid & (W - 1);                       // vertex of this lane
    const int base = g << a.wshift;                    // first thread of the group
    const int64_t row = (int64_t)blockIdx.x * (UGS_WL_BLOCK >> a.wshift) + g;
    const bool row_ok = row < a.rows;
    const int T = a.iterations;

    // ---- vertices and neighbour masks ----
    const int64_t id = row_ok && u < a.k ? a.nodes[row * a.k + u] : -1;
    const bool valid = id >= 0;
    const u64 gmask = W == 32 ? 0xffffffffull : ((1ull << W) - 1ull);
    const int gshift = (tid & 63) - u;                 // the group's first lane inside the wave
    const u64 ballot = __ballot(valid);
    const int n = __popcll((ballot >> gshift) & gmask);
    mask_sh[tid] = 0;
    if (u == 0) bad_sh[g] = 0;
    __syncthreads();
    if (row_ok && n > 0) {
        const int64_t lo = a.edge_ptr[row], hi = a.edge_ptr[row + 1];
        if (lo < 0 || hi < lo || hi > a.num_cols) {
            if (u == 0) bad_sh[g] = 1;                 // not a range of edge_index: refused like a bad endpoint, nothing is read
        } else {
            for (int64_t e = lo + u; e < hi; e += W) {
                const int64_t x = a.edge_index[e], y = a.edge_index[a.stride + e];
                if (x < 0 || x >= n || y < 0 || y >= n) {
                    bad_sh[g] = 1;
                } else {
                    atomicOr(&mask_sh[base + (int)x], 1u << (int)y);
                    atomicOr(&mask_sh[base + (int)y], 1u << (int)x);
                }
            }
        }
    }
    // ---- label mode: the j-th valid slot of the row is vertex j and brings labels[id] as the top 32 bits of the high word ----
    bool norange = false;
    if (a.labeled) {
        bool out = false;
        if (valid) {
            const int64_t l = id < a.num_labels ? a.labels[id] : -1;
            out = (u64)l > 0xffffffffull;              // an id past the label rows, or a label outside [0, 2^32)
            if (!out) {
                const int j = __popcll((ballot >> gshift) & ((1ull << u) - 1ull));
                lab_sh[0][base + j][0] = (u64)l << 32;
                lab_sh[0][base + j][1] = 0;
            }
        }
        norange = ((__ballot(out) >> gshift) & gmask) != 0ull;
    }
    __syncthreads();
    const int st = !row_ok ? -1 : n == 0 ? 1 : bad_sh[g] ? 2 : norange ? 3 : 0;
    const bool live = st == 0 && u < n;                // this lane hashes a vertex
    const unsigned mymask = live ? mask_sh[tid] : 0u;

    // ---- start labels: str(degree), a loop counting twice ----
    if (live && !a.labeled) {
        unsigned len;
        const u64 d = dec2((unsigned)__popc(mymask) + ((mymask >> u) & 1u), &len);
        lab_sh[0][tid][0] = ((d & 0xffull) << 56) | ((d >> 8) << 48);
        lab_sh[0][tid][1] = 0;
    }
    int cur = 0;
    WlStream fs;                                       // the final string's stream: lane 0 of the group
    wl_stream_init(fs);
    unsigned nitems = 0;
    u64 *const stg = &stg_sh[tid];
    u64 *const fstg = &fstg_sh[g];

    for (int t = 0; t <= T; ++t) {
        // ---- order[]: the labels of buffer `cur` ranked, ties by vertex; cnt[rank] = multiplicity at the first of equal labels ----
        __syncthreads();
        if (live) {
            const u64 hi = lab_sh[cur][tid][0], lo = lab_sh[cur][tid][1];
            int rank = 0, eq_before = 0, eq_all = 0;
            for (int v = 0; v < n; ++v) {
                const u64 h2 = lab_sh[cur][base + v][0], l2 = lab_sh[cur][base + v][1];
                const bool eq = h2 == hi && l2 == lo;
                const bool less = h2 < hi || (h2 == hi && l2 < lo);
                rank += (less || (eq && v < u)) ? 1 : 0;
                eq_before += (eq && v < u) ? 1 : 0;
                eq_all += eq ? 1 : 0;
            }
            order_sh[base + rank] = (unsigned char)u;
            cnt_sh[base + rank] = (unsigned char)(eq_before == 0 ? eq_all : 0);
        }
        __syncthreads();

        // ---- the final string takes this iteration's items (t >= 1), and after the last iteration its end ----
        if (st == 0 && u == 0) {
            const bool closing = t == T;
            const int items = t >= 1 ? n : 0;
            for (int r = 0; r < items + (closing ? 1 : 0); ++r) {
                const bool tail = r == items;
                const unsigned c = tail ? 0u : cnt_sh[base + r];
                if (!tail && c == 0u) continue;
                const int src = tail ? base : base + order_sh[base + r];
                const u64 hi = lab_sh[cur][src][0], lo = lab_sh[cur][src][1];
                for (int p = 0; p < (tail ? 3 : 6); ++p) {
                    int what = WL_PIECE;
                    u64 v = 0;
                    unsigned len = 0;
                    if (tail) {
                        if (p == 0) {                  // "()" for no items, ",)" after a single one, ")" otherwise
                            if (nitems == 0u) { v = (u64)'(' | ((u64)')' << 8); len = 2; }
                            else if (nitems == 1u) { v = (u64)',' | ((u64)')' << 8); len = 2; }
                            else { v = (u64)')'; len = 1; }
                        } else {
                            what = p == 1 ? WL_FLUSH : WL_FINISH;
                        }
                    } else if (p == 0) {
                        if (nitems == 0u) { v = (u64)'(' | ((u64)'(' << 8) | ((u64)'\'' << 16); len = 3; }
                        else { v = (u64)',' | ((u64)' ' << 8) | ((u64)'(' << 16) | ((u64)'\'' << 24); len = 4; }
                    } else if (p <= 4) {
                        v = hex8(hex_word(hi, lo, p - 1));
                        len = 8;
                    } else {                           // "', <count>)"
                        unsigned dl;
                        const u64 d = dec2(c, &dl);
                        v = (u64)'\'' | ((u64)',' << 8) | ((u64)' ' << 16) | (d << 24) | ((u64)')' << (24 + 8 * dl));
                        len = 4 + dl;
                        ++nitems;
                    }
                    wl_stream_step(fs, fstg, UGS_WL_BLOCK / 8, what, v, len);
                }
            }
        }
        if (t == T) break;

        // ---- vertex messages of iteration t + 1: own label, then the neighbours' labels in sorted order ----
        if (live) {
            WlStream s;
            wl_stream_init(s);
            const bool dec = t == 0 && !a.labeled;     // decimal start labels: one piece each; hex labels: four pieces of 8 characters,
            const int ppl_shift = t == 0 ? 0 : 2;      // 32-bit start labels of label mode: one piece of 8 characters
            const int steps = ((n + 1) << ppl_shift) + 2;
            for (int j = 0; j < steps; ++j) {
                const int li = j >> ppl_shift, p = j & ((1 << ppl_shift) - 1);
                int what = WL_PIECE;
                u64 v = 0;
                unsigned len = 0;
                if (li > n) {
                    what = j == steps - 2 ? WL_FLUSH : WL_FINISH;
                } else {
                    int src = tid;
                    if (li > 0) {
                        const int w = order_sh[base + li - 1];
                        if (!((mymask >> w) & 1u)) continue;
                        src = base + w;
                    }
                    const u64 hi = lab_sh[cur][src][0], lo = lab_sh[cur][src][1];
                    if (dec) {
                        v = (hi >> 56) | (((hi >> 48) & 0xffull) << 8);
                        len = (hi >> 48) & 0xffull ? 2u : 1u;
                    } else {
                        v = hex8(hex_word(hi, lo, p));
                        len = 8;
                    }
                }
                wl_stream_step(s, stg, UGS_WL_BLOCK, what, v, len);
            }
            lab_sh[cur ^ 1][tid][0] = __builtin_bswap64(s.h[0]);      // digest bytes 0-7 and 8-15, big-endian: hex order = integer order
            lab_sh[cur ^ 1][tid][1] = __builtin_bswap64(s.h[1]);
        }
        cur ^= 1;
    }

    if (row_ok && u == 0) {
        a.digest[row * 2] = st == 0 ? __builtin_bswap64(fs.h[0]) : 0;
        a.digest[row * 2 + 1] = st == 0 ? __builtin_bswap64(fs.h[1]) : 0;
        a.status[row] = st;
    }
}

struct WlLookupArgs {
    const u64 *digest;           // [rows, 2]
    const int32_t *status;       // [rows]
    int64_t rows;
    const u64 *keys;             // [vocab, 2] ascending as 128-bit values
    const int64_t *ids;          // [vocab]
    int64_t vocab, unknown_id;
    int64_t *out;                // [rows]
};

__global__ __launch_bounds__(256) void ugs_wl_lookup_kernel(WlLookupArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.rows) return;
    int64_t id = a.unknown_id;
    if (a.status[i] == 0) {
        const u64 hi = a.digest[2 * i], lo = a.digest[2 * i + 1];
        int64_t lo_i = 0, hi_i = a.vocab;               // first key >= the digest
        while (lo_i < hi_i) {
            const int64_t mid = lo_i + ((hi_i - lo_i) >> 1);
            const u64 kh = a.keys[2 * mid], kl = a.keys[2 * mid + 1];
            if (kh < hi || (kh == hi && kl < lo)) lo_i = mid + 1; else hi_i = mid;
        }
        if (lo_i < a.vocab && a.keys[2 * lo_i] == hi && a.keys[2 * lo_i + 1] == lo) id = a.ids[lo_i];
    }
    a.out[i] = id;
}

}  // namespace

static int wl_hash_launch(const int64_t *d_nodes, const int64_t *d_edge_index, int64_t row_stride, int64_t num_cols, const int64_t *d_edge_ptr,
                          int64_t rows, int k, int iterations, int labeled, const int64_t *d_labels, int64_t num_labels, uint64_t *d_digest,
                          int32_t *d_status) {
    if (k < 1 || k > UGS_KMAX) return ugs_internal_fail(UGS_E_UNSUPPORTED, "wl_hash: 1 <= k <= 32");
    if (iterations < 0 || iterations > UGS_WL_MAX_ITER) return ugs_internal_fail(UGS_E_UNSUPPORTED, "wl_hash: 0 <= iterations <= 8");
    if (rows < 0 || num_cols < 0 || (num_cols > 0 && row_stride < num_cols)) return ugs_internal_fail(UGS_E_BAD_ARG, "wl_hash: rows >= 0, num_cols >= 0, row_stride >= num_cols");
    if (num_labels < 0) return ugs_internal_fail(UGS_E_BAD_ARG, "wl_hash: num_labels >= 0");
    if (rows == 0) return UGS_OK;
    if (!d_nodes || !d_edge_ptr || !d_digest || !d_status || (num_cols > 0 && !d_edge_index) || (num_labels > 0 && !d_labels))
        return ugs_internal_fail(UGS_E_BAD_ARG, "wl_hash: null pointer");
    hipStream_t s = nullptr;
    if (int rc = ugs_internal_ctx(nullptr, &s)) return rc;
    WlHashArgs a{};
    a.nodes = d_nodes; a.edge_index = d_edge_index; a.stride = row_stride; a.num_cols = num_cols; a.edge_ptr = d_edge_ptr;
    a.rows = rows; a.k = k; a.iterations = iterations;
    a.wshift = k <= 8 ? 3 : k <= 16 ? 4 : 5;
    a.digest = reinterpret_cast<u64 *>(d_digest); a.status = d_status;
    a.labels = d_labels; a.num_labels = num_labels; a.labeled = labeled;
    const int64_t per_block = UGS_WL_BLOCK >> a.wshift;
    const int64_t blocks = (rows + per_block - 1) / per_block;
    if (blocks > 0x7fffffffll) return ugs_internal_fail(UGS_E_UNSUPPORTED, "wl_hash: too many rows for one launch");
    hipLaunchKernelGGL(ugs_wl_hash_kernel, dim3((unsigned)blocks), dim3(UGS_WL_BLOCK), 0, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ugs_internal_fail(UGS_E_HIP, hipGetErrorString(e));
    return UGS_OK;
}

extern "C" int ugs_wl_hash(const int64_t *d_nodes, const int64_t *d_edge_index, int64_t row_stride, int64_t num_cols,
                           const int64_t *d_edge_ptr, int64_t rows, int k, int iterations, uint64_t *d_digest, int32_t *d_status) {
    return wl_hash_launch(d_nodes, d_edge_index, row_stride, num_cols, d_edge_ptr, rows, k, iterations, 0, nullptr, 0, d_digest, d_status);
}

extern "C" int ugs_wl_hash_labeled(const int64_t *d_nodes, const int64_t *d_edge_index, int64_t row_stride, int64_t num_cols,
                                   const int64_t *d_edge_ptr, int64_t rows, int k, int iterations, const int64_t *d_labels,
                                   int64_t num_labels, uint64_t *d_digest, int32_t *d_status) {
    return wl_hash_launch(d_nodes, d_edge_index, row_stride, num_cols, d_edge_ptr, rows, k, iterations, 1, d_labels, num_labels, d_digest, d_status);
}

extern "C" int ugs_wl_feature_labels(const void *d_x, int64_t row_bytes, int64_t row_stride_bytes, int64_t num_rows, int64_t *d_labels) {
    if (row_bytes < 0 || num_rows < 0 || row_stride_bytes < row_bytes)
        return ugs_internal_fail(UGS_E_BAD_ARG, "wl_feature_labels: row_bytes >= 0, num_rows >= 0, row_stride_bytes >= row_bytes");
    if (row_bytes >= (1ll << 29)) return ugs_internal_fail(UGS_E_UNSUPPORTED, "wl_feature_labels: row_bytes < 2^29");
    if (num_rows == 0) return UGS_OK;
    if (!d_labels || (row_bytes > 0 && !d_x)) return ugs_internal_fail(UGS_E_BAD_ARG, "wl_feature_labels: null pointer");
    const int64_t blocks = (num_rows + 255) / 256;
    if (blocks > 0x7fffffffll) return ugs_internal_fail(UGS_E_UNSUPPORTED, "wl_feature_labels: too many rows for one launch");
    hipStream_t s = nullptr;
    if (int rc = ugs_internal_ctx(nullptr, &s)) return rc;
    WlLabelArgs a{};
    a.x = static_cast<const unsigned char *>(d_x); a.stride = row_stride_bytes; a.rows = num_rows; a.len = (unsigned)row_bytes; a.labels = d_labels;
    hipLaunchKernelGGL(ugs_wl_feature_labels_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ugs_internal_fail(UGS_E_HIP, hipGetErrorString(e));
    return UGS_OK;
}

extern "C" int ugs_wl_lookup(const uint64_t *d_digest, const int32_t *d_status, int64_t rows, const uint64_t *d_keys,
                             const int64_t *d_ids, int64_t vocab_size, int64_t unknown_id, int64_t *d_ids_out) {
    if (rows < 0 || vocab_size < 0) return ugs_internal_fail(UGS_E_BAD_ARG, "wl_lookup: rows >= 0 and vocab_size >= 0");
    if (rows == 0) return UGS_OK;
    if (!d_digest || !d_status || !d_ids_out || (vocab_size > 0 && (!d_keys || !d_ids))) return ugs_internal_fail(UGS_E_BAD_ARG, "wl_lookup: null pointer");
    const int64_t blocks = (rows + 255) / 256;
    if (blocks > 0x7fffffffll) return ugs_internal_fail(UGS_E_UNSUPPORTED, "wl_lookup: too many rows for one launch");
    hipStream_t s = nullptr;
    if (int rc = ugs_internal_ctx(nullptr, &s)) return rc;
    WlLookupArgs a{};
    a.digest = reinterpret_cast<const u64 *>(d_digest); a.status = d_status; a.rows = rows;
    a.keys = reinterpret_cast<const u64 *>(d_keys); a.ids = d_ids; a.vocab = vocab_size; a.unknown_id = unknown_id; a.out = d_ids_out;
    hipLaunchKernelGGL(ugs_wl_lookup_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ugs_internal_fail(UGS_E_HIP, hipGetErrorString(e));
    return UGS_OK;
}
