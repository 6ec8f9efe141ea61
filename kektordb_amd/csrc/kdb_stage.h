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

// A region of a KdbStage: where it starts and what it takes.  An absent region (bytes == 0) reads as a null device pointer -- what
// the launchers take for "optional, not given".
struct KdbRegion {
    size_t off = 0, bytes = 0;
    template <typename T>
    T *at(unsigned char *base) const { return bytes ? reinterpret_cast<T *>(base + off) : nullptr; }
};

// The regions of one staged call, each DECLARED ONCE: its bytes, and the host pointer it is filled from (in) or delivered to (out).
// Built on the carver, so the order of the declarations is still the layout.  An input or output whose host pointer is null or
// whose size is 0 is absent: it takes nothing (take(0)) and is never copied.  dev() is a region only the device uses -- or one the
// caller copies piece by piece itself.  copy_in / copy_out make one copy per present region, in declaration order, through
// copy(dst, src, bytes) -> 0 or an error code that ends the walk (the library: hipMemcpyAsync on the turn's stream; the test: memcpy).
struct KdbStage {
    static constexpr int CAP = 8; // (the consensus call has eight regions)
    struct Slot {
        KdbRegion r;
        const void *src;
        void *dst;
    };
    KdbCarver cv;
    Slot slots[CAP];
    int n = 0;
    bool overflow = false; // more than CAP declarations: total() is still right, the copies refuse

    KdbRegion in(const void *src, size_t bytes) { return add(src ? bytes : 0, src, nullptr); }
    KdbRegion out(void *dst, size_t bytes) { return add(dst ? bytes : 0, nullptr, dst); }
    KdbRegion dev(size_t bytes) { return add(bytes, nullptr, nullptr); }
    size_t total() const { return cv.total(); }

    template <typename Copy>
    int copy_in(unsigned char *base, Copy copy) const {
        if (overflow) return -1;
        for (int i = 0; i < n; i++)
            if (slots[i].src && slots[i].r.bytes)
                if (const int rc = copy(static_cast<void *>(base + slots[i].r.off), slots[i].src, slots[i].r.bytes)) return rc;
        return 0;
    }
    template <typename Copy>
    int copy_out(unsigned char *base, Copy copy) const {
        if (overflow) return -1;
        for (int i = 0; i < n; i++)
            if (slots[i].dst && slots[i].r.bytes)
                if (const int rc = copy(slots[i].dst, static_cast<const void *>(base + slots[i].r.off), slots[i].r.bytes)) return rc;
        return 0;
    }

  private:
    KdbRegion add(size_t bytes, const void *src, void *dst) {
        KdbRegion r;
        r.off = cv.take(bytes);
        r.bytes = bytes;
        if (n < CAP) slots[n++] = Slot{r, src, dst};
        else overflow = true;
        return r;
    }
};
