// kdb_stage.h -- how a staging buffer is cut into regions (host only: no HIP header, tests/cpp/stage_layout_test.cpp builds it alone).
#pragma once
#include <stddef.h>
#include <stdint.h>

// bytes of a dense bitset over the ids 0..n (allow lists, active lists): whole 64-bit words
static inline size_t kdb_bits_bytes(uint32_t n) { return ((size_t)(n >> 6) + 1) * 8; }

// One buffer, carved front to back: the ORDER of the take() calls is the layout.  Every region starts on a 256-byte boundary; an
// empty one (an optional input that is absent) takes nothing and shares its offset with the region behind it.
struct KdbCarver {
    size_t at = 0;
    size_t take(size_t bytes) {
        const size_t o = at;
        at += (bytes + 255) & ~(size_t)255;
        return o;
    }
    size_t total() const { return at; } // what the buffer must hold
};
