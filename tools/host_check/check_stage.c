/* tools/host_check -- the staging planner of the outputs that leave as several host destinations from one launch (ovhip_stage_plan_,
 * openvvc_amd/csrc/ovvc_outdst_priv.h: what ovhip_pic_output_ladder, _ladder_lut and _rgb_pyramid lay their scratch out with) as a
 * stand-alone program.  Every array the planner reads or writes -- destinations, bytes given, bytes needed, offsets -- is a heap block of
 * exactly n elements, and the destinations are carved out of one heap block of exactly their bytes, so that a read or a write one
 * element outside is the sanitizer's to see.  1 and 8 items; sizes that are and are not multiples of 256; a destination one byte
 * short; a null destination; a size of 0; two destinations that overlap by 2 bytes, reported as (k, j); destinations that touch.
 * `make asan`.  Host code only. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "ovvc_outdst_priv.h"

typedef struct { int n; void **dst; size_t *given, *need, *off; uint8_t *mem; } items;

/* n destinations of need[k] bytes behind one another in one block, touching: item k begins where item k - 1 ends */
static items
make(int n, const size_t *need)
{
    items it = { n, malloc(n * sizeof(void *)), malloc(n * sizeof(size_t)), malloc(n * sizeof(size_t)), malloc(n * sizeof(size_t)), NULL };
    size_t all = 0;
    for (int k = 0; k < n; ++k) all += need[k];
    it.mem = (uint8_t *)malloc(all ? all : 1);
    if (!it.dst || !it.given || !it.need || !it.off || !it.mem) exit(2);
    all = 0;
    for (int k = 0; k < n; ++k) { it.dst[k] = it.mem + all; it.given[k] = it.need[k] = need[k]; all += need[k]; it.off[k] = (size_t)-1; }
    return it;
}

static void drop(items *it) { free(it->dst); free(it->given); free(it->need); free(it->off); free(it->mem); }

static long n_plans;

/* the plan of `it` answers `want`; OK: the offsets and the total are the 256-byte layout; else: the items it names are (wk, wj; -1: any) */
static int
expect(const items *it, int want, int wk, int wj, const char *what)
{
    size_t total = (size_t)-1;
    int k = -1, j = -1;
    const int r = ovhip_stage_plan_(it->n, it->dst, it->given, it->need, it->off, &total, &k, &j);
    int bad = r != want;
    if (!bad && want == OVHIP_STAGE_OK_) {
        size_t at = 0;
        for (int i = 0; i < it->n && !bad; ++i) {
            bad = it->off[i] != at || (at & 255);
            at += (it->need[i] + 255) / 256 * 256;
        }
        bad = bad || total != at;
    } else if (!bad)
        bad = k != wk || (want == OVHIP_STAGE_OVERLAP_ && j != wj);
    if (bad) fprintf(stderr, "%s: %d (wanted %d), items (%d, %d) (wanted (%d, %d)), total %zu\n", what, r, want, k, j, wk, wj, total);
    ++n_plans;
    return bad;
}

int
main(void)
{
    static const size_t one_even[1] = { 4096 }, one_odd[1] = { 4097 }, one_small[1] = { 1 };
    static const size_t eight[8] = { 256, 255, 257, 1, 98304, 61441, 512, 12345 };      /* multiples of 256 and not; every pair touches */
    int bad = 0;
    {
        items a = make(1, one_even), b = make(1, one_odd), c = make(1, one_small);
        bad |= expect(&a, OVHIP_STAGE_OK_, -1, -1, "one item, a multiple of 256") | expect(&b, OVHIP_STAGE_OK_, -1, -1, "one item, no multiple of 256")
               | expect(&c, OVHIP_STAGE_OK_, -1, -1, "one item of one byte");
        a.given[0] -= 1;
        bad |= expect(&a, OVHIP_STAGE_UNFIT_, 0, -1, "one item, one byte short");
        b.dst[0] = NULL;
        bad |= expect(&b, OVHIP_STAGE_UNFIT_, 0, -1, "one item, no destination");
        c.need[0] = 0;
        bad |= expect(&c, OVHIP_STAGE_UNFIT_, 0, -1, "one item, no size");
        drop(&a); drop(&b); drop(&c);
    }
    {
        items e = make(8, eight);
        bad |= expect(&e, OVHIP_STAGE_OK_, -1, -1, "eight items that touch");
        for (int k = 0; k < 8; ++k) e.given[k] += 7;                             /* more than needed is fine; the plan goes by the need */
        bad |= expect(&e, OVHIP_STAGE_OK_, -1, -1, "eight items given more than they need");
        drop(&e);
    }
    for (int k = 0; k < 8; ++k) {
        items e = make(8, eight);
        e.given[k] = eight[k] - 1;
        bad |= expect(&e, OVHIP_STAGE_UNFIT_, k, -1, "eight items, one a byte short");
        e.given[k] = eight[k]; e.dst[k] = NULL;
        bad |= expect(&e, OVHIP_STAGE_UNFIT_, k, -1, "eight items, one without a destination");
        drop(&e);
    }
    /* One of items j < k moved so that its first 2 bytes are the other's last 2: the pair is reported as (k, j) whichever of the two was
     * moved, since the later item is asked against the earlier ones, the earliest first.  (The items in front of j end where j began, at
     * least 2 bytes in front of the moved item; the moved item may reach into items behind the other one, which are asked later.  Items
     * of fewer than 3 bytes stay where they are: moved, they would lie inside the other) */
    for (int k = 1; k < 8; ++k)
        for (int j = 0; j < k; ++j) {
            if (eight[k] < 3 || eight[j] < 3) continue;
            items e = make(8, eight);
            e.dst[k] = (uint8_t *)e.dst[j] + eight[j] - 2;
            bad |= expect(&e, OVHIP_STAGE_OVERLAP_, k, j, "eight items, a later one 2 bytes into an earlier one");
            drop(&e);
            e = make(8, eight);
            e.dst[j] = (uint8_t *)e.dst[k] + eight[k] - 2;
            bad |= expect(&e, OVHIP_STAGE_OVERLAP_, k, j, "eight items, an earlier one 2 bytes into a later one");
            drop(&e);
        }
    {   /* an unfit item in front of an overlapping pair is the answer, and the other way round: the items are asked in order */
        items e = make(8, eight);
        e.dst[5] = (uint8_t *)e.dst[4] + eight[4] - 2; e.dst[2] = NULL;
        bad |= expect(&e, OVHIP_STAGE_UNFIT_, 2, -1, "unfit item 2 in front of the overlapping pair (5, 4)");
        e.dst[2] = e.mem + eight[0] + eight[1]; e.given[7] = 0;
        bad |= expect(&e, OVHIP_STAGE_OVERLAP_, 5, 4, "the overlapping pair (5, 4) in front of unfit item 7");
        drop(&e);
    }
    if (bad) return 1;
    printf("check_stage: %ld plans: offsets on 256-byte boundaries, unfit items and overlapping pairs named in order\n", n_plans);
    return 0;
}
