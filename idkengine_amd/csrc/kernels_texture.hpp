// kernels_texture.hpp — decode-at-upload of the storage formats a host really holds (include/idkpt.h, IDKPT_TEXFMT_R8 .. BC7_SRGBA) into one of the three RESIDENT formats
// the sampler reads (tex_fetch, pt_kernels.hpp): the bytes cross PCIe as the engine keeps them, one kernel expands them once, nothing stays compressed on the device.
// Part of the single translation unit idkpt.hip.  The block / texel decoders are plain inline functions: this header also compiles under a host C++ compiler (no HIP), where
// TEXFN is `inline` and the tables are ordinary constants — a CPU build can step through them under gdb or a host sanitizer; the __global__ kernels exist under hipcc only.
#pragma once
#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#define TEXFN __device__ inline
#define TEXTABLE __constant__ const
#else
#define TEXFN inline
#define TEXTABLE static const
#endif

namespace texdec {

TEXFN float bits_to_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

// ---- R11G11B10F (GL 4.6 2.3.4.3 / 2.3.4.4: unsigned 11- and 10-bit floats): 5-bit exponent (bias 15), M-bit mantissa.  Every finite value is exact in binary32.
TEXFN float ufloat_decode(uint32_t v, int M)
{
    const uint32_t e = v >> M, m = v & ((1u << M) - 1u);
    if (e == 0) return (float)m * (M == 6 ? 9.5367431640625e-07f /* 2^-20 */ : 1.9073486328125e-06f /* 2^-19 */);   // m / 2^M * 2^-14
    if (e == 31) return bits_to_float(m ? 0x7fc00000u : 0x7f800000u);
    return bits_to_float(((e + 112u) << 23) | (m << (23 - M)));
}
TEXFN void r11g11b10f_decode(uint32_t w, float out[4])
{
    out[0] = ufloat_decode(w & 0x7ffu, 6); out[1] = ufloat_decode((w >> 11) & 0x7ffu, 6); out[2] = ufloat_decode(w >> 22, 5); out[3] = 1.0f;
}

// ---- BC4 / each half of BC5 (RGTC1 unsigned): r0, r1, 48 bits of 3-bit codes; texel i = x + 4y.  The stored float is the GL formula's real value rounded ONCE:
// integer numerator / (7 * 255) or (5 * 255) — r0, r1 and the constants 0 / 1 go through the same expression (255 -> exactly 1.0f).
TEXFN float rgtc_texel(uint64_t block, int i)
{
    const uint32_t r0 = (uint32_t)(block & 0xff), r1 = (uint32_t)((block >> 8) & 0xff), k = (uint32_t)((block >> (16 + 3 * i)) & 7);
    if (r0 > r1) {
        const uint32_t num = k == 0 ? 7u * r0 : (k == 1 ? 7u * r1 : (8u - k) * r0 + (k - 1u) * r1);
        return (float)num / 1785.0f;
    }
    const uint32_t num = k == 0 ? 5u * r0 : (k == 1 ? 5u * r1 : (k == 6 ? 0u : (k == 7 ? 1275u : (6u - k) * r0 + (k - 1u) * r1)));
    return (float)num / 1275.0f;
}

// ---- BC7 (BPTC UNORM: ARB_texture_compression_bptc / Khronos Data Format 1.3, BPTC): the result is defined to the bit.
// per mode: subsets | partition bits << 2 | rotation bits << 5 | index-selection bit << 7 | colour bits << 8 | alpha bits << 12 | p-bit kind << 16 (0 none, 1 per endpoint,
// 2 shared per subset) | index bits << 18 | second index bits << 21
#define BC7_MODE_WORD(ns, pb, rb, isb, cb, ab, pm, ib, ib2) ((uint32_t)(ns) | ((pb) << 2) | ((rb) << 5) | ((isb) << 7) | ((cb) << 8) | ((ab) << 12) | ((pm) << 16) | ((ib) << 18) | ((ib2) << 21))
TEXTABLE uint32_t BC7_MODES[8] = {
    BC7_MODE_WORD(3, 4, 0, 0, 4, 0, 1, 3, 0), BC7_MODE_WORD(2, 6, 0, 0, 6, 0, 2, 3, 0), BC7_MODE_WORD(3, 6, 0, 0, 5, 0, 0, 2, 0), BC7_MODE_WORD(2, 6, 0, 0, 7, 0, 1, 2, 0),
    BC7_MODE_WORD(1, 0, 2, 1, 5, 6, 0, 2, 3), BC7_MODE_WORD(1, 0, 2, 0, 7, 8, 0, 2, 2), BC7_MODE_WORD(1, 0, 0, 0, 7, 7, 1, 4, 0), BC7_MODE_WORD(2, 6, 0, 0, 5, 5, 1, 2, 0)};
// two-subset partitions: bit i = subset of texel i
TEXTABLE uint16_t BC7_PART2[64] = {
    0xcccc, 0x8888, 0xeeee, 0xecc8, 0xc880, 0xfeec, 0xfec8, 0xec80, 0xc800, 0xffec, 0xfe80, 0xe800, 0xffe8, 0xff00, 0xfff0, 0xf000,
    0xf710, 0x008e, 0x7100, 0x08ce, 0x008c, 0x7310, 0x3100, 0x8cce, 0x088c, 0x3110, 0x6666, 0x366c, 0x17e8, 0x0ff0, 0x718e, 0x399c,
    0xaaaa, 0xf0f0, 0x5a5a, 0x33cc, 0x3c3c, 0x55aa, 0x9696, 0xa55a, 0x73ce, 0x13c8, 0x324c, 0x3bdc, 0x6996, 0xc33c, 0x9966, 0x0660,
    0x0272, 0x04e4, 0x4e40, 0x2720, 0xc936, 0x936c, 0x39c6, 0x639c, 0x9336, 0x9cc6, 0x817e, 0xe718, 0xccf0, 0x0fcc, 0x7744, 0xee22};
// three-subset partitions: bits [2i, 2i + 1] = subset of texel i
TEXTABLE uint32_t BC7_PART3[64] = {
    0xaa685050, 0x6a5a5040, 0x5a5a4200, 0x5450a0a8, 0xa5a50000, 0xa0a05050, 0x5555a0a0, 0x5a5a5050, 0xaa550000, 0xaa555500, 0xaaaa5500, 0x90909090, 0x94949494, 0xa4a4a4a4, 0xa9a59450, 0x2a0a4250,
    0xa5945040, 0x0a425054, 0xa5a5a500, 0x55a0a0a0, 0xa8a85454, 0x6a6a4040, 0xa4a45000, 0x1a1a0500, 0x0050a4a4, 0xaaa59090, 0x14696914, 0x69691400, 0xa08585a0, 0xaa821414, 0x50a4a450, 0x6a5a0200,
    0xa9a58000, 0x5090a0a8, 0xa8a09050, 0x24242424, 0x00aa5500, 0x24924924, 0x24499224, 0x50a50a50, 0x500aa550, 0xaaaa4444, 0x66660000, 0xa5a0a5a0, 0x50a050a0, 0x69286928, 0x44aaaa44, 0x66666600,
    0xaa444444, 0x54a854a8, 0x95809580, 0x96969600, 0xa85454a8, 0x80959580, 0xaa141414, 0x96960000, 0xaaaa1414, 0xa05050a0, 0xa0a5a5a0, 0x96000000, 0x40804080, 0xa9a8a9a8, 0xaaaaaa44, 0x2a4a5254};
// anchor texels (the index stored with one bit fewer) besides texel 0: two-subset partitions: of subset 1; three-subset partitions: of subset 1 | of subset 2 << 4
TEXTABLE uint8_t BC7_ANCHOR2[64] = {
    15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 2, 8, 2, 2, 8, 8, 15, 2, 8, 2, 2, 8, 8, 2, 2,
    15, 15, 6, 8, 2, 8, 15, 15, 2, 8, 2, 2, 2, 15, 15, 6, 6, 2, 6, 8, 15, 15, 2, 2, 15, 15, 15, 15, 15, 2, 2, 15};
TEXTABLE uint8_t BC7_ANCHOR3[64] = {
    0xf3, 0x83, 0x8f, 0x3f, 0xf8, 0xf3, 0x3f, 0x8f, 0xf8, 0xf8, 0xf6, 0xf6, 0xf6, 0xf5, 0xf3, 0x83, 0xf3, 0x83, 0xf8, 0x3f, 0xf3, 0x83, 0xf6, 0x8a, 0x35, 0xf8, 0x68, 0xa6, 0xf8, 0xf5, 0xaf, 0x8f,
    0xf8, 0x3f, 0xf3, 0xa5, 0xa6, 0x8a, 0x98, 0xaf, 0x6f, 0xf3, 0x8f, 0xf5, 0x3f, 0x6f, 0x6f, 0x8f, 0xf3, 0x3f, 0xf5, 0xf5, 0xf5, 0xf8, 0xf5, 0xfa, 0xf5, 0xfa, 0xf8, 0xfd, 0x3f, 0xfc, 0xf3, 0x83};

// n bits of the 128-bit little-endian block from bit *pos on (n <= 8: a field never needs more than two words), advancing *pos
TEXFN uint32_t bc7_bits(uint64_t lo, uint64_t hi, uint32_t* pos, uint32_t n)
{
    const uint32_t p = *pos; *pos = p + n;
    uint64_t v;
    if (p >= 64) v = hi >> (p - 64);
    else v = p == 0 ? lo : ((lo >> p) | (hi << (64 - p)));
    return (uint32_t)v & ((1u << n) - 1u);
}
// interpolation weights of 2-, 3- and 4-bit indices, one byte each
TEXFN uint32_t bc7_weight(uint32_t bits, uint32_t i)
{
    if (bits == 2) return (0x402b1500u >> (8 * i)) & 0xff;                                   // 0 21 43 64
    if (bits == 3) return (uint32_t)(0x40372e251b120900ull >> (8 * i)) & 0xff;               // 0 9 18 27 37 46 55 64
    return (uint32_t)((i < 8 ? 0x1e1a15110d090400ull : 0x403c37332f2b2622ull) >> (8 * (i & 7))) & 0xff;   // 0 4 9 13 17 21 26 30 | 34 38 43 47 51 55 60 64
}
TEXFN uint32_t bc7_lerp(uint32_t e0, uint32_t e1, uint32_t w) { return ((64u - w) * e0 + w * e1 + 32u) >> 6; }

// One block -> 16 texels, texel i = x + 4y, packed R | G << 8 | B << 16 | A << 24.  The header (mode, partition, endpoints, p-bits) is parsed once; endpoints and indices live in
// packed words (no dynamically indexed array: every loop below has a constant trip count and unrolls into registers).
TEXFN void bc7_decode_block(uint64_t lo, uint64_t hi, uint32_t out[16])
{
    const uint32_t b0 = (uint32_t)(lo & 0xff);
    if (b0 == 0) {                                                      // reserved: (0, 0, 0, 0)
#pragma unroll
        for (int i = 0; i < 16; i++) out[i] = 0u;
        return;
    }
    uint32_t mode = 0; while (!((b0 >> mode) & 1u)) mode++;
    const uint32_t mw = BC7_MODES[mode];
    const uint32_t ns = mw & 3u, pb = (mw >> 2) & 7u, rb = (mw >> 5) & 3u, isb = (mw >> 7) & 1u, cb = (mw >> 8) & 15u, ab = (mw >> 12) & 15u, pm = (mw >> 16) & 3u, ib = (mw >> 18) & 7u, ib2 = (mw >> 21) & 3u;
    uint32_t pos = mode + 1u;
    const uint32_t part = bc7_bits(lo, hi, &pos, pb), rot = bc7_bits(lo, hi, &pos, rb), sel = bc7_bits(lo, hi, &pos, isb);
    const uint32_t ne = 2u * ns;
    uint32_t ep[6] = {0u, 0u, 0u, 0u, 0u, 0u};                         // endpoint 2s / 2s + 1 of subset s: raw fields, one byte per channel
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const uint32_t n = c < 3 ? cb : ab;
#pragma unroll
        for (int e = 0; e < 6; e++) if ((uint32_t)e < ne && n) ep[e] |= bc7_bits(lo, hi, &pos, n) << (8 * c);
    }
    uint32_t pbits = 0;                                                 // bit e: p-bit of endpoint e
    if (pm == 1) pbits = bc7_bits(lo, hi, &pos, ne);
    else if (pm == 2) { const uint32_t s = bc7_bits(lo, hi, &pos, ns); pbits = (s & 1u) * 3u | ((s >> 1) & 1u) * 12u | ((s >> 2) & 1u) * 48u; }
    const uint32_t cprec = cb + (pm ? 1u : 0u), aprec = ab + (pm && ab ? 1u : 0u);
#pragma unroll
    for (int e = 0; e < 6; e++) {
        uint32_t w = 0;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            uint32_t v = (ep[e] >> (8 * c)) & 0xff; const uint32_t prec = c < 3 ? cprec : aprec;
            if (c == 3 && ab == 0) v = 255u;
            else { if (pm) v = (v << 1) | ((pbits >> e) & 1u); v <<= 8u - prec; v |= v >> prec; }   // left shift + replication of the high bits
            w |= (v & 0xff) << (8 * c);
        }
        ep[e] = w;
    }
    uint32_t smap = 0, a1 = 0, a2 = 0;                                  // subset of texel i in bits [2i, 2i + 1]; the anchors besides texel 0 (0: none)
    if (ns == 2) { const uint32_t m = BC7_PART2[part]; a1 = BC7_ANCHOR2[part];
#pragma unroll
        for (int i = 0; i < 16; i++) smap |= ((m >> i) & 1u) << (2 * i);
    } else if (ns == 3) { smap = BC7_PART3[part]; a1 = BC7_ANCHOR3[part] & 15u; a2 = BC7_ANCHOR3[part] >> 4; }
    uint64_t idx1 = 0, idx2 = 0;                                        // 4 bits per texel
#pragma unroll
    for (int i = 0; i < 16; i++) { const bool anchor = i == 0 || (a1 && (uint32_t)i == a1) || (a2 && (uint32_t)i == a2); idx1 |= (uint64_t)bc7_bits(lo, hi, &pos, ib - (anchor ? 1u : 0u)) << (4 * i); }
    if (ib2) {
#pragma unroll
        for (int i = 0; i < 16; i++) idx2 |= (uint64_t)bc7_bits(lo, hi, &pos, ib2 - (i == 0 ? 1u : 0u)) << (4 * i);
    }
    // which index set and width interpolates colour / alpha (modes 4, 5: two sets; the index-selection bit of mode 4 swaps them)
    const uint32_t cbits = ib2 && sel ? ib2 : ib, abits = ib2 && !sel ? ib2 : ib;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const uint32_t s = (smap >> (2 * i)) & 3u;
        const uint32_t e0 = s == 0 ? ep[0] : (s == 1 ? ep[2] : ep[4]), e1 = s == 0 ? ep[1] : (s == 1 ? ep[3] : ep[5]);
        const uint32_t i1 = (uint32_t)(idx1 >> (4 * i)) & 15u, i2 = (uint32_t)(idx2 >> (4 * i)) & 15u;
        const uint32_t wc = bc7_weight(cbits, ib2 && sel ? i2 : i1), wa = bc7_weight(abits, ib2 && !sel ? i2 : i1);
        uint32_t r = bc7_lerp(e0 & 0xff, e1 & 0xff, wc), g = bc7_lerp((e0 >> 8) & 0xff, (e1 >> 8) & 0xff, wc), b = bc7_lerp((e0 >> 16) & 0xff, (e1 >> 16) & 0xff, wc);
        uint32_t a = ab ? bc7_lerp(e0 >> 24, e1 >> 24, wa) : 255u;
        if (rot == 1) { const uint32_t t = a; a = r; r = t; } else if (rot == 2) { const uint32_t t = a; a = g; g = t; } else if (rot == 3) { const uint32_t t = a; a = b; b = t; }
        out[i] = r | (g << 8) | (b << 16) | (a << 24);
    }
}

}   // namespace texdec

#ifdef __HIPCC__
// ---- one __global__ per source family.  Every store is bounds-checked against width x height; the source sizes are what the host validated (host_scene.hpp, tex_source_bytes).

// R8 / RG8 -> RGBA8 (r, g | 0, 0, 255); R11G11B10F -> RGBA32F (r, g, b, 1): one texel per thread, contiguous stores
__global__ void k_tex_expand_linear(const uint8_t* src, void* dst, size_t texels, int format)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= texels) return;
    if (format == IDKPT_TEXFMT_R8) ((uint32_t*)dst)[t] = (uint32_t)src[t] | 0xff000000u;
    else if (format == IDKPT_TEXFMT_RG8) { const uint32_t rg = ((const uint16_t*)src)[t]; ((uint32_t*)dst)[t] = rg | 0xff000000u; }
    else { float v[4]; texdec::r11g11b10f_decode(((const uint32_t*)src)[t], v); ((float4*)dst)[t] = make_float4(v[0], v[1], v[2], v[3]); }
}

// BC4 (8-byte blocks) / BC5 (16-byte blocks: R block, G block) -> RGBA32F (r, g | 0, 0, 1): one texel per thread (the 4 lanes of a block row share its 8 / 16 bytes), contiguous 16-byte stores
__global__ void k_tex_decode_rgtc(const uint64_t* src, float4* dst, int w, int h, int two)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)w * h) return;
    const int x = (int)(t % (size_t)w), y = (int)(t / (size_t)w), i = (x & 3) + 4 * (y & 3);
    const size_t blk = (size_t)(y >> 2) * ((w + 3) >> 2) + (x >> 2);
    const float r = texdec::rgtc_texel(src[two ? 2 * blk : blk], i), g = two ? texdec::rgtc_texel(src[2 * blk + 1], i) : 0.0f;
    dst[t] = make_float4(r, g, 0.0f, 1.0f);
}

// BC7 -> RGBA8 bytes (the resident format says UNORM or sRGB): one block per thread — its header is parsed once — and one 16-byte store per texel row of the block, so the 64
// horizontally adjacent blocks of a wave write 1 KB of contiguous RGBA8 per row.  Edge blocks / widths that are no multiple of 4 store texel by texel, inside the image only.
__global__ void k_tex_decode_bc7(const uint4* src, uint32_t* dst, int w, int h)
{
    const int bw = (w + 3) >> 2, bh = (h + 3) >> 2;
    const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= (size_t)bw * bh) return;
    const int bx = (int)(b % (size_t)bw), by = (int)(b / (size_t)bw);
    const uint4 q = src[b];
    uint32_t px[16];
    texdec::bc7_decode_block((uint64_t)q.x | ((uint64_t)q.y << 32), (uint64_t)q.z | ((uint64_t)q.w << 32), px);
    const int x0 = 4 * bx, y0 = 4 * by;
    const bool whole = (w & 3) == 0 && y0 + 4 <= h;                    // (w % 4 == 0: x0 + 4 <= w, and every row start is 16-byte aligned)
#pragma unroll
    for (int y = 0; y < 4; y++) {
        uint32_t* row = dst + (size_t)(y0 + y) * w + x0;
        if (whole) *(uint4*)row = make_uint4(px[4 * y], px[4 * y + 1], px[4 * y + 2], px[4 * y + 3]);
        else if (y0 + y < h) {
#pragma unroll
            for (int x = 0; x < 4; x++) if (x0 + x < w) row[x] = px[4 * y + x];
        }
    }
}
#endif
