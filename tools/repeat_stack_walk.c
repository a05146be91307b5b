/* The textbook pass that grlbwt_fm_repeats replaces, for tools/gpu_fm_repeats.py --route-b: one serial stack walk over the LCP
 * array (4-byte values) that visits every LCP interval -- every right-maximal repeat -- once and counts those whose value lies in
 * [min_len, max_len].  stack: room for 2 * (largest value + 2) words (the values on the stack ascend strictly).
 * No left-maximality, no table: the least the host route has to do. */
#include <stdint.h>

uint64_t repeat_stack_walk(const uint32_t *lcp, uint64_t n, uint32_t min_len, uint32_t max_len, uint64_t *stack) {
    uint64_t top = 0, found = 0;                   /* entries (value, left boundary) */
    stack[0] = 0; stack[1] = 0; top = 1;
    for (uint64_t p = 1; p <= n; p++) {
        const uint64_t v = p < n ? lcp[p] : 0;
        uint64_t left = p - 1;
        while (top && stack[2 * (top - 1)] > v) {
            const uint64_t len = stack[2 * (top - 1)];
            left = stack[2 * (top - 1) + 1];
            top--;
            if (len >= min_len && len <= max_len) found++;      /* the interval [left, p) of value len */
        }
        if (!top || stack[2 * (top - 1)] < v) { stack[2 * top] = v; stack[2 * top + 1] = left; top++; }
    }
    return found;
}
