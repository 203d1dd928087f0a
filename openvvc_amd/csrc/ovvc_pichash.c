/* Decoded picture hash SEI (payload type 132) on the host: the three methods over planes in host memory, the payload reader the
 * reference does not have (nvcl_nal_sei.c knows the number and skips the payload), and the comparison.  Definitions:
 * include/ovvc_hip.h, "Decoded picture hash"; the device half is kernels_pichash.hip.  Plain C, no device. */
#include <string.h>
#include "ovvc_hip.h"

/* one byte into the register of (0x1021, most significant bit first) without its 16 closing steps: crc' = (crc x^8 + b x^16) mod P */
static inline uint32_t
crc_byte(uint32_t crc, uint32_t b)
{
    uint32_t x = (crc >> 8) ^ b;
    x ^= x >> 4;
    return ((crc << 8) ^ (x << 12) ^ (x << 5) ^ x) & 0xFFFF;
}

static uint32_t
plane_crc(const uint16_t *p, int w, int h, int stride)
{
    /* this form of the register ends at (start x^n + M x^16) mod P: the 16 closing steps are already in it, and the definition's start
     * value enters as 0xFFFF x^16 mod P = 0x1D0F */
    uint32_t crc = 0x1D0F;
    for (int y = 0; y < h; ++y) {
        const uint16_t *row = p + (size_t)y * stride;
        for (int x = 0; x < w; ++x) crc = crc_byte(crc_byte(crc, row[x] & 0xFF), row[x] >> 8);
    }
    return crc;
}

static uint32_t
plane_checksum(const uint16_t *p, int w, int h, int stride)
{
    uint32_t sum = 0;
    for (int y = 0; y < h; ++y) {
        const uint16_t *row = p + (size_t)y * stride;
        const uint32_t my = ((uint32_t)y & 0xFF) ^ ((uint32_t)y >> 8);
        for (int x = 0; x < w; ++x) {
            const uint32_t m = my ^ ((uint32_t)x & 0xFF) ^ ((uint32_t)x >> 8), s = row[x];
            sum += ((s & 0xFF) ^ m) + ((s >> 8) ^ m);
        }
    }
    return sum;
}

static void
plane_md5(const uint16_t *p, int w, int h, int stride, uint8_t out[16])
{
    ovhip_md5_state st;
    ovhip_md5_init(&st);
    uint8_t buf[512];
    for (int y = 0; y < h; ++y) {
        const uint16_t *row = p + (size_t)y * stride;
        for (int x = 0; x < w; ) {
            int n = 0;
            for (; n < 256 && x < w; ++n, ++x) { buf[2 * n] = (uint8_t)(row[x] & 0xFF); buf[2 * n + 1] = (uint8_t)(row[x] >> 8); }
            ovhip_md5_update(&st, buf, 2 * (size_t)n);
        }
    }
    ovhip_md5_final(&st, out);
}

static int value_bytes(int method) { return method == OVHIP_HASH_MD5 ? 16 : (method == OVHIP_HASH_CRC ? 2 : 4); }

int
ovhip_pic_hash_host(int method, int n_planes, const uint16_t *y, const uint16_t *cb, const uint16_t *cr, int32_t w, int32_t h,
                    int32_t stride_y, int32_t stride_c, ovhip_pic_hash_value *out)
{
    if (!out || method < OVHIP_HASH_MD5 || method > OVHIP_HASH_CHECKSUM || (n_planes != 1 && n_planes != 3)) return OVHIP_EINVAL;
    if (!y || w <= 0 || h <= 0 || (w & 1) || (h & 1) || stride_y < w) return OVHIP_EINVAL;
    if (n_planes == 3 && (!cb || !cr || stride_c < w / 2)) return OVHIP_EINVAL;
    memset(out, 0, sizeof(*out));
    out->method = (uint8_t)method; out->n_planes = (uint8_t)n_planes;
    for (int c = 0; c < n_planes; ++c) {
        const uint16_t *p = c == 0 ? y : (c == 1 ? cb : cr);
        const int pw = c ? w / 2 : w, ph = c ? h / 2 : h, ps = c ? stride_c : stride_y;
        uint8_t *v = out->value[c];
        if (method == OVHIP_HASH_MD5) plane_md5(p, pw, ph, ps, v);
        else if (method == OVHIP_HASH_CRC) { const uint32_t r = plane_crc(p, pw, ph, ps); v[0] = (uint8_t)(r >> 8); v[1] = (uint8_t)r; }
        else { const uint32_t r = plane_checksum(p, pw, ph, ps); v[0] = (uint8_t)(r >> 24); v[1] = (uint8_t)(r >> 16); v[2] = (uint8_t)(r >> 8); v[3] = (uint8_t)r; }
    }
    return OVHIP_OK;
}

int
ovhip_pic_hash_parse_sei(const uint8_t *payload, size_t n, ovhip_pic_hash_value *out)
{
    if (!payload || !out || n < 2 || payload[0] > OVHIP_HASH_CHECKSUM) return OVHIP_EINVAL;
    const int method = payload[0], n_planes = (payload[1] & 0x80) ? 1 : 3, nb = value_bytes(method);
    if (n < 2 + (size_t)n_planes * (size_t)nb) return OVHIP_EINVAL;
    memset(out, 0, sizeof(*out));
    out->method = (uint8_t)method; out->n_planes = (uint8_t)n_planes;
    for (int c = 0; c < n_planes; ++c) memcpy(out->value[c], payload + 2 + c * nb, (size_t)nb);
    return OVHIP_OK;
}

int
ovhip_pic_hash_equal(const ovhip_pic_hash_value *a, const ovhip_pic_hash_value *b)
{
    if (!a || !b || a->method != b->method || a->n_planes != b->n_planes || a->method > OVHIP_HASH_CHECKSUM || a->n_planes > 3) return 0;
    for (int c = 0; c < a->n_planes; ++c)
        if (memcmp(a->value[c], b->value[c], (size_t)value_bytes(a->method))) return 0;
    return 1;
}
