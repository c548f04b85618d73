// carve.h -- a call's pieces of one grow-only buffer, each with its size (no HIP here: tests/carve_check.cpp builds with the
// system compiler).  `pieces(Carve &)` takes them all and runs twice (carve_pieces): first without a base, to add up the sizes --
// the buffer grows once, before anything is enqueued (growing moves it) -- then to hand out the pointers.
#pragma once
#include <cstddef>
#include <cstdint>

// `n` elements of T at `p` (device memory).  Where a kernel wants the pointer, the piece converts to it.
template <class T> struct Piece {
    T *p = nullptr;
    size_t n = 0;
    size_t bytes() const { return n * sizeof(T); }
    operator T *() const { return p; }
};

struct Carve {
    char *base = nullptr;
    size_t align = 256;    // a power of two: every piece starts at a multiple of it
    size_t off = 0;
    bool overflow = false; // a size did not fit size_t: the pieces from there on are empty and carve_pieces fails
    // `count` elements of T -- none (a null piece of size 0, no space taken) unless `want`
    template <class T> Piece<T> take(size_t count, bool want = true)
    {
        if (!want || overflow) return {};
        const size_t a = align - 1;
        if (count > (SIZE_MAX - a) / sizeof(T) || ((count * sizeof(T) + a) & ~a) > SIZE_MAX - off) { overflow = true; return {}; }
        Piece<T> piece{base ? reinterpret_cast<T *>(base + off) : nullptr, count};
        off += (count * sizeof(T) + a) & ~a;
        return piece;
    }
};

// buf: ensure(bytes) -> 0 when it holds that many, as<char>() -> its base.  -> false: the sizes overflow or the buffer did not grow
template <class Buf, class F> bool carve_pieces(Buf &buf, size_t align, F &&pieces)
{
    Carve c{nullptr, align};
    pieces(c);
    if (c.overflow || buf.ensure(c.off)) return false;
    c = Carve{buf.template as<char>(), align};
    pieces(c);
    return true;
}
