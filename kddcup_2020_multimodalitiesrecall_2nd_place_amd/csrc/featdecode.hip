// Box features of TSV records decoded on the device (mms_decode_feats_b64, include/mmscore.h): the base64 text of a record's
// 6th field (f32 [num_boxes, 2048] row-major) -> its zero-padded [10, 2048] fp32 row, bit for bit what libmmfeat's b64_decode writes
// (csrc/featurizer.cpp), so the host only gathers the raw text (mmf_gather_spans) and the PCIe copy carries ~42 KB per record instead of 80 KB.
//
// Layout: 16 base64 characters are 12 bytes are 3 whole floats.  A record's text starts 16-byte aligned, so unit u of a record is ONE
// 128-bit load of characters 16u .. 16u+15 and 3 floats stored at 3u; consecutive lanes cover contiguous bytes on both sides.  One
// workgroup per record: its lanes walk the units of the record's live rows, then zero rows [rows, 10) with 16-byte stores.
//
// Validation follows the host decoder: it decodes exactly rows x 8192 bytes, i.e. reads the first ceil(rows x 8192 x 4 / 3) characters,
// and any of them outside A-Z a-z 0-9 + / ('=' included) fails the record.  Characters past that count -- the rest of the last unit's
// load, the text of rows past the 10th -- are neither validated nor decoded into a written byte.
#include "kernels.h"

namespace {

constexpr int FD_THREADS = 256;
constexpr int FD_ROW_BYTES = MMS_FEAT * 4;                 // decoded bytes per box row
constexpr int FD_ROW_FLOAT4 = MMS_NBOX * MMS_FEAT / 4;     // 16-byte stores per padded record

// 6-bit value of one base64 character (standard alphabet); anything else sets `bad`
__device__ __forceinline__ uint32_t b64_value(uint32_t c, uint32_t& bad) {
    const bool up = c - 'A' < 26u, low = c - 'a' < 26u, dig = c - '0' < 10u, plus = c == '+', slash = c == '/';
    bad |= (up | low | dig | plus | slash) ? 0u : 1u;
    return up ? c - 'A' : low ? c - 'a' + 26u : dig ? c - '0' + 52u : plus ? 62u : 63u;
}

__global__ __launch_bounds__(FD_THREADS) void k_decode_feats_b64(const char* chars, const int64_t* char_off, const int32_t* rows_in,
                                                                 float* feats, int32_t* bad) {
    const int64_t i = blockIdx.x;
    const int64_t off = char_off[i];
    const bool aligned = off >= 0 && (off & 15) == 0;
    int rows = rows_in[i];
    rows = rows < 0 || !aligned ? 0 : rows > MMS_NBOX ? MMS_NBOX : rows;      // a misaligned / negative start: nothing is read, the record is flagged
    const int nbytes = rows * FD_ROW_BYTES;
    const int nchars = (nbytes * 4 + 2) / 3;
    const int units = (nbytes + 11) / 12;
    const uint4* src = reinterpret_cast<const uint4*>(chars + (aligned ? off : 0));
    uint32_t* dst = reinterpret_cast<uint32_t*>(feats + i * (int64_t)(MMS_NBOX * MMS_FEAT));
    uint32_t flag = aligned ? 0u : 1u;
    for (int u = threadIdx.x; u < units; u += FD_THREADS) {
        const uint4 q = src[u];
        const uint32_t w4[4] = {q.x, q.y, q.z, q.w};
        const int live = nchars - 16 * u;                  // characters of this unit that the host decoder reads (>= 16 but in the last unit)
        uint32_t x[4];                                     // four 24-bit groups
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            uint32_t acc = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int j = 4 * g + k;
                const uint32_t c = (w4[g] >> (8 * k)) & 0xFFu;
                uint32_t b = 0;
                const uint32_t v = b64_value(c, b);
                acc = (acc << 6) | (j < live ? v : 0u);
                flag |= j < live ? b : 0u;
            }
            x[g] = acc;
        }
        // bytes 3g .. 3g+2 = x[g] >> 16, >> 8, >> 0; word k = bytes 4k .. 4k+3, little endian
        const uint32_t b0 = x[0] >> 16 & 0xFF, b1 = x[0] >> 8 & 0xFF, b2 = x[0] & 0xFF;
        const uint32_t b3 = x[1] >> 16 & 0xFF, b4 = x[1] >> 8 & 0xFF, b5 = x[1] & 0xFF;
        const uint32_t b6 = x[2] >> 16 & 0xFF, b7 = x[2] >> 8 & 0xFF, b8 = x[2] & 0xFF;
        const uint32_t b9 = x[3] >> 16 & 0xFF, b10 = x[3] >> 8 & 0xFF, b11 = x[3] & 0xFF;
        const uint32_t w0 = b0 | b1 << 8 | b2 << 16 | b3 << 24;
        const uint32_t w1 = b4 | b5 << 8 | b6 << 16 | b7 << 24;
        const uint32_t w2 = b8 | b9 << 8 | b10 << 16 | b11 << 24;
        uint32_t* d = dst + 3 * u;
        const int words = (nbytes - 12 * u) >> 2;          // 3, or 1 / 2 in a record's last unit (nbytes is a multiple of 4)
        if (words >= 3) {
            d[0] = w0; d[1] = w1; d[2] = w2;
        } else {
            d[0] = w0;
            if (words == 2) d[1] = w1;
        }
    }
    uint4* z = reinterpret_cast<uint4*>(dst);             // rows [rows, 10): rows x 2048 floats is a multiple of 4
    for (int k = rows * (MMS_FEAT / 4) + threadIdx.x; k < FD_ROW_FLOAT4; k += FD_THREADS) z[k] = make_uint4(0u, 0u, 0u, 0u);
    const int any = __syncthreads_or((int)flag);
    if (threadIdx.x == 0) bad[i] = any ? 1 : 0;
}

}  // namespace

void launch_decode_feats_b64(const char* chars, const int64_t* char_off, const int32_t* rows, long long B, float* feats, int32_t* bad, hipStream_t st) {
    if (B > 0) hipLaunchKernelGGL(k_decode_feats_b64, dim3((unsigned)B), dim3(FD_THREADS), 0, st, chars, char_off, rows, feats, bad);
}
