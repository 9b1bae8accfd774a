// stream_order.h -- the one ordering rule of the stream schedules (plain C++17, no HIP: tests/test_stream_order.py compiles it on the host).
//
// A stream of calls (the *_loop and *_batch entries, the public submit) enqueues call i + 1's speculative first attempt -- Gram pass,
// Cholesky with its verdict, an apply pass that skips itself on rejection -- BEFORE call i is finished.  When call i is rejected, its
// ladder runs after that attempt.  That is still the blocking order only when the two calls do not touch each other's memory:
//   * Q(i) or R(i) overlaps A(i + 1): attempt i + 1 factors what was there before call i's ladder wrote it;
//   * Q(i) or R(i) overlaps Q(i + 1) or R(i + 1): call i's ladder writes after call i + 1, the blocking order leaves call i + 1's result;
//   * Q(i + 1) or R(i + 1) overlaps A(i): attempt i + 1 writes over the input call i's ladder is about to read.
// Such a pair CONFLICTS: call i is finished before call i + 1 is enqueued.  A call's own in-place operands (q == a) are no conflict, nor
// are two A's that only read the same memory.  Operands are compared as whole byte ranges ((n - 1) ld + rows elements), so an operand in
// the padding rows of another's columns (ld > rows) counts as overlapping: conservative, never too loose.
#ifndef TSQR_STREAM_ORDER_H
#define TSQR_STREAM_ORDER_H
#include <cstddef>
#include <cstdint>

namespace tsqr_order {

// byte range of a column-major rows x n operand with leading dimension ld
struct Range {
	std::uintptr_t lo = 0, hi = 0;                   // [lo, hi)
	Range() = default;
	Range(const void* p, std::size_t ld, std::size_t rows, std::size_t n, std::size_t esz)
	    : lo(reinterpret_cast<std::uintptr_t>(p)), hi(lo + (n == 0 ? 0 : ((n - 1) * ld + rows) * esz)) {}
	bool overlaps(const Range& o) const { return lo < o.hi && o.lo < hi && lo < hi && o.lo < o.hi; }
};

// the operands of one call
struct Operands {
	Range q, r, a;
};
inline Operands operands(const void* q, std::size_t ldq, const void* r, std::size_t ldr, const void* a, std::size_t lda,
                         std::size_t m, std::size_t n, std::size_t esz) {
	return Operands{Range(q, ldq, m, n, esz), Range(r, ldr, n, n, esz), Range(a, lda, m, n, esz)};
}

// an output of call i is memory call j reads (Q(i) or R(i) overlaps A(j)).  Applied to one call against itself it tells whether a loop
// over one triple feeds each call's result into the next call.
inline bool feeds(const Operands& i, const Operands& j) { return i.q.overlaps(j.a) || i.r.overlaps(j.a); }

// calls i and i + 1 conflict: call i must be finished before call i + 1's attempt is enqueued
inline bool conflict(const Operands& i, const Operands& next) {
	return feeds(i, next) || feeds(next, i) ||
	       i.q.overlaps(next.q) || i.q.overlaps(next.r) || i.r.overlaps(next.q) || i.r.overlaps(next.r);
}

}  // namespace tsqr_order
#endif
