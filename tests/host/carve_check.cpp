// carve_check.cpp -- adapted_amd/csrc/carve.h on the host alone (no HIP): the sizing pass and the pointer pass agree, every piece
// is aligned and inside the buffer, an unwanted piece is null and takes nothing, and sizes that do not fit size_t fail instead
// of wrapping.  Built with -fsanitize=address,undefined and run by tests/test_carve_cpu.py; exit status 0 = all held.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "carve.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("carve_check.cpp:%d: %s\n", __LINE__, #cond); failures++; } } while (0)

// a grow-only host buffer with DevBuf's interface; `limit`: the most it will hold
struct HostBuf {
    char *p = nullptr;
    size_t cap = 0, limit = (size_t)1 << 30, asked = 0;
    int calls = 0;
    ~HostBuf() { std::free(p); }
    int ensure(size_t bytes)
    {
        calls++; asked = bytes;
        if (bytes > limit) return -1;
        if (bytes <= cap) return 0;
        std::free(p);
        p = static_cast<char *>(std::aligned_alloc(256, (bytes + 255) & ~(size_t)255));
        cap = p ? bytes : 0;
        return p ? 0 : -1;
    }
    template <class T> T *as() { return reinterpret_cast<T *>(p); }
};

struct Span { const char *lo, *hi; };
struct Row { char bytes[544]; }; // (a size that is no multiple of either alignment)

// a call's pieces of mixed types and sizes, some unwanted; every wanted one is written to its last byte (ASan checks the bounds)
static void check_call(size_t align, size_t n, size_t cap, bool staged)
{
    HostBuf buf;
    Piece<char> sig, none; Piece<int32_t> len, info; Piece<int64_t> pos; Piece<double> vals; Piece<Row> rows; Piece<uint8_t> one;
    size_t sized = 0;
    int pass = 0;
    const bool ok = carve_pieces(buf, align, [&](Carve &w) {
        sig = w.take<char>(n * 1000 * 4, staged);
        len = w.take<int32_t>(n); pos = w.take<int64_t>(n * cap); info = w.take<int32_t>(n * 5);
        none = w.take<char>(12345, false);
        vals = w.take<double>(n * 3); rows = w.take<Row>(n); one = w.take<uint8_t>(1);
        if (pass++ == 0) { sized = w.off; CHECK(!w.base && !len.p && len.n == n); } // (the sizing pass: counts, no pointers)
        else CHECK(w.off == sized && w.base == buf.p);
    });
    CHECK(ok && pass == 2 && buf.calls == 1 && buf.asked == sized && sized <= buf.cap);
    CHECK(none.p == nullptr && none.n == 0 && none.bytes() == 0);
    CHECK(staged ? (sig.p == buf.p && sig.n == n * 4000) : (sig.p == nullptr && sig.n == 0 && (char *)len.p == buf.p));
    CHECK(len.n == n && pos.n == n * cap && info.n == n * 5 && vals.n == n * 3 && rows.n == n && one.n == 1);
    CHECK(info.bytes() == n * 20 && vals.bytes() == n * 24 && rows.bytes() == n * 544);
    std::vector<Span> spans;
    auto add = [&](const void *p, size_t bytes) {
        if (!p) return;
        const char *c = static_cast<const char *>(p);
        CHECK(((uintptr_t)c & (align - 1)) == 0);
        CHECK(c >= buf.p && c + bytes <= buf.p + sized);
        for (const Span &s : spans) CHECK(c >= s.hi || c + bytes <= s.lo);
        spans.push_back({c, c + bytes});
        for (size_t i = 0; i < bytes; i++) const_cast<char *>(c)[i] = (char)i;
    };
    add(sig.p, sig.bytes()); add(len.p, len.bytes()); add(pos.p, pos.bytes()); add(info.p, info.bytes());
    add(vals.p, vals.bytes()); add(rows.p, rows.bytes()); add(one.p, one.bytes());
    CHECK(spans.size() == (staged ? 7u : 6u));
    // an empty piece that is wanted: a valid pointer of no elements, no space
    Carve c{buf.p, align};
    const Piece<double> z = c.take<double>(0);
    CHECK(z.p == (double *)buf.p && z.n == 0 && c.off == 0);
}

template <class T> static void check_overflow(size_t align)
{
    const size_t most = SIZE_MAX / sizeof(T);
    for (size_t count : {most, most - 1, most + 1, most - align / sizeof(T), (size_t)SIZE_MAX, most / 2 + 1}) {
        if (count < most / 2) continue; // (most + 1 of a one-byte type is 0)
        // alone: too large only where the aligned size does not fit
        Carve a{nullptr, align};
        const Piece<T> p = a.take<T>(count);
        const bool fits = count <= (SIZE_MAX - (align - 1)) / sizeof(T);
        CHECK(a.overflow == !fits);
        if (fits) CHECK(p.n == count && a.off >= count * sizeof(T) && a.off % align == 0);
        else CHECK(p.p == nullptr && p.n == 0 && a.off == 0);
        // behind another piece, twice over: the sum does not fit
        HostBuf buf;
        buf.limit = SIZE_MAX;
        Piece<T> first, second; Piece<char> after;
        const bool ok = carve_pieces(buf, align, [&](Carve &w) {
            first = w.take<T>(most / 2 + 1); second = w.take<T>(count); after = w.take<char>(1);
        });
        CHECK(!ok && buf.calls == 0 && second.n == 0 && after.n == 0 && after.p == nullptr);
    }
}

int main()
{
    for (size_t align : {(size_t)16, (size_t)256})
        for (size_t n : {(size_t)1, (size_t)3, (size_t)64, (size_t)1000})
            for (int staged = 0; staged < 2; staged++) check_call(align, n, 3, staged != 0);
    check_overflow<char>(16); check_overflow<char>(256);
    check_overflow<int32_t>(256); check_overflow<double>(16); check_overflow<double>(256); check_overflow<Row>(256);
    // a buffer that does not grow: no pointers are handed out
    HostBuf small;
    small.limit = 1000;
    int passes = 0;
    CHECK(!carve_pieces(small, 256, [&](Carve &w) { (void)w.take<double>(1000); passes++; }) && passes == 1 && small.calls == 1);
    // the same call twice on one buffer takes the same memory; a smaller one does not shrink it
    HostBuf again;
    Piece<double> a1, a2;
    CHECK(carve_pieces(again, 256, [&](Carve &w) { (void)w.take<char>(7); a1 = w.take<double>(100); }));
    CHECK(carve_pieces(again, 256, [&](Carve &w) { (void)w.take<char>(7); a2 = w.take<double>(10); }));
    CHECK(a1.p == a2.p && (char *)a1.p == again.p + 256 && again.cap == 256 + 1024);
    std::printf(failures ? "carve_check: %d checks failed\n" : "carve_check: ok\n", failures);
    return failures ? 1 : 0;
}
