/* Stand-alone check of the decoded picture hash's host code (see the Makefile): ovhip_pic_hash_host against the vector table of
 * include/ovvc_hip.h's definitions and against the definitions written out bit by bit here, and ovhip_pic_hash_parse_sei on payloads
 * of exactly their length and one byte less.  Every buffer is a heap block of exactly the bytes it may be read for. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "ovvc_hip.h"

static int n_fail;
#define CHECK(c, ...) do { if (!(c)) { ++n_fail; fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

/* s(x, y, c) = (37x + 101y + 7xy + 13c + ((x ^ y) << 3)) & 1023, or full 16-bit noise */
static uint16_t *
make_plane(int w, int h, int stride, int c, int noise)
{
    uint16_t *p = (uint16_t *)malloc(((size_t)(h - 1) * stride + w) * sizeof(*p));       /* the last row ends at its last sample */
    uint32_t lcg = 12345u + (uint32_t)c * 77u + (uint32_t)w;
    if (!p) exit(2);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < stride && (y < h - 1 || x < w); ++x) {
            lcg = lcg * 1664525u + 1013904223u;
            p[(size_t)y * stride + x] = noise || x >= w ? (uint16_t)(lcg >> 13) : (uint16_t)((37 * x + 101 * y + 7 * x * y + 13 * c + ((x ^ y) << 3)) & 1023);
        }
    return p;
}

static uint32_t
crc_literal(const uint16_t *p, int w, int h, int stride)
{
    uint32_t crc = 0xFFFF;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const uint32_t s = p[(size_t)y * stride + x], bytes[2] = { s & 0xFF, s >> 8 };
            for (int b = 0; b < 2; ++b)
                for (int k = 7; k >= 0; --k) {
                    const uint32_t top = crc >> 15;
                    crc = ((crc << 1) | ((bytes[b] >> k) & 1)) & 0xFFFF;
                    if (top) crc ^= 0x1021;
                }
        }
    for (int k = 0; k < 16; ++k) { const uint32_t top = crc >> 15; crc = (crc << 1) & 0xFFFF; if (top) crc ^= 0x1021; }
    return crc;
}

static uint32_t
sum_literal(const uint16_t *p, int w, int h, int stride)
{
    uint32_t sum = 0;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const uint32_t s = p[(size_t)y * stride + x], m = (uint32_t)((x & 0xFF) ^ (y & 0xFF) ^ (x >> 8) ^ (y >> 8));
            sum += ((s & 0xFF) ^ m) + ((s >> 8) ^ m);
        }
    return sum;
}

static void
md5_literal(const uint16_t *p, int w, int h, int stride, uint8_t out[16])
{
    ovhip_md5_state st;
    ovhip_md5_init(&st);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const uint8_t b[2] = { (uint8_t)(p[(size_t)y * stride + x] & 0xFF), (uint8_t)(p[(size_t)y * stride + x] >> 8) };
            ovhip_md5_update(&st, b, 2);
        }
    ovhip_md5_final(&st, out);
}

static const struct { int w, h; uint32_t crc[3], sum[3]; const char *md5_y; } VEC[] = {
    { 8, 8, { 0xe55b, 0xf7bd, 0x5c5b }, { 0x00001ee1, 0x00000794, 0x0000085c }, "a91c7749a0e42e7239fcae6fe49af8ec" },
    { 24, 8, { 0x6cee, 0xaa8e, 0xb34e }, { 0x0000696e, 0x00001a27, 0x0000198a }, "add3795b4791364bb3eb949be76768f5" },
    { 72, 40, { 0x77d5, 0xb12f, 0x458f }, { 0x0007403a, 0x0001a5cd, 0x00019ea0 }, "7ce24f75b803002a905dbe9177b49457" },
    { 520, 264, { 0xfd3d, 0x9ee0, 0xe37c }, { 0x0215d6af, 0x00857bc2, 0x008515bf }, "52f5e941ffc9cbec15ab67395442611c" },
    { 8, 520, { 0, 0, 0 }, { 0, 0, 0 }, NULL },                           /* (no table entry: against the literal forms only) */
};

static void
one_picture(int w, int h, int pad, int noise, int vec)
{
    const int sy = w + pad, sc = w / 2 + pad;
    uint16_t *pl[3] = { make_plane(w, h, sy, 0, noise), make_plane(w / 2, h / 2, sc, 1, noise), make_plane(w / 2, h / 2, sc, 2, noise) };
    for (int method = 0; method <= 2; ++method)
        for (int n_planes = 1; n_planes <= 3; n_planes += 2) {
            ovhip_pic_hash_value v;
            memset(&v, 0xEE, sizeof(v));
            const int r = ovhip_pic_hash_host(method, n_planes, pl[0], n_planes == 3 ? pl[1] : NULL, n_planes == 3 ? pl[2] : NULL, w, h, sy, sc, &v);
            CHECK(r == OVHIP_OK && v.method == method && v.n_planes == n_planes, "%dx%d method %d planes %d: %d", w, h, method, n_planes, r);
            uint8_t want[3][16];
            memset(want, 0, sizeof(want));
            for (int c = 0; c < n_planes; ++c) {
                const int pw = c ? w / 2 : w, ph = c ? h / 2 : h, ps = c ? sc : sy;
                if (method == OVHIP_HASH_MD5) md5_literal(pl[c], pw, ph, ps, want[c]);
                else if (method == OVHIP_HASH_CRC) {
                    const uint32_t q = crc_literal(pl[c], pw, ph, ps);
                    want[c][0] = (uint8_t)(q >> 8); want[c][1] = (uint8_t)q;
                    if (vec >= 0 && !noise && VEC[vec].md5_y) CHECK(q == VEC[vec].crc[c], "%dx%d CRC plane %d: %04x, table %04x", w, h, c, q, VEC[vec].crc[c]);
                } else {
                    const uint32_t q = sum_literal(pl[c], pw, ph, ps);
                    want[c][0] = (uint8_t)(q >> 24); want[c][1] = (uint8_t)(q >> 16); want[c][2] = (uint8_t)(q >> 8); want[c][3] = (uint8_t)q;
                    if (vec >= 0 && !noise && VEC[vec].md5_y) CHECK(q == VEC[vec].sum[c], "%dx%d checksum plane %d: %08x, table %08x", w, h, c, q, VEC[vec].sum[c]);
                }
            }
            CHECK(!memcmp(v.value, want, sizeof(want)), "%dx%d method %d planes %d pad %d noise %d: value differs from the definition", w, h, method, n_planes, pad, noise);
            if (method == OVHIP_HASH_MD5 && vec >= 0 && !noise && VEC[vec].md5_y) {
                char hex[33];
                for (int i = 0; i < 16; ++i) snprintf(hex + 2 * i, 3, "%02x", v.value[0][i]);
                CHECK(!strcmp(hex, VEC[vec].md5_y), "%dx%d MD5 Y: %s, table %s", w, h, hex, VEC[vec].md5_y);
            }
            /* the value as an SEI payload of exactly its length, read back; one byte less is refused */
            const int nb = method == OVHIP_HASH_MD5 ? 16 : (method == OVHIP_HASH_CRC ? 2 : 4);
            const size_t n = 2 + (size_t)n_planes * nb;
            uint8_t *payload = (uint8_t *)malloc(n), *shorter = (uint8_t *)malloc(n - 1);
            if (!payload || !shorter) exit(2);
            payload[0] = (uint8_t)method; payload[1] = n_planes == 1 ? 0x80 : 0x00;
            for (int c = 0; c < n_planes; ++c) memcpy(payload + 2 + c * nb, v.value[c], (size_t)nb);
            memcpy(shorter, payload, n - 1);
            ovhip_pic_hash_value back;
            CHECK(ovhip_pic_hash_parse_sei(payload, n, &back) == OVHIP_OK && ovhip_pic_hash_equal(&back, &v) == 1 && !memcmp(&back, &v, sizeof(v)),
                  "%dx%d method %d planes %d: payload round trip", w, h, method, n_planes);
            CHECK(ovhip_pic_hash_parse_sei(shorter, n - 1, &back) == OVHIP_EINVAL, "a payload one byte short was accepted");
            payload[0] = 3;
            CHECK(ovhip_pic_hash_parse_sei(payload, n, &back) == OVHIP_EINVAL, "hash type 3 was accepted");
            free(payload); free(shorter);
        }
    for (int c = 0; c < 3; ++c) free(pl[c]);
}

int
main(void)
{
    for (int i = 0; i < (int)(sizeof(VEC) / sizeof(VEC[0])); ++i)
        for (int noise = 0; noise < 2; ++noise)
            for (int pad = 0; pad <= 5; pad += 5) one_picture(VEC[i].w, VEC[i].h, pad, noise, i);
    printf("check_pichash: %s\n", n_fail ? "FAILED" : "ok");
    return n_fail != 0;
}
