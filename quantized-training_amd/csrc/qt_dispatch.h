// qt_dispatch.h -- host only: where a run-time fact (format kind, stage count, "is there an amax slot", an element-format pair)
// becomes a template argument.  Each picker hands the matching value to a generic lambda as a std::integral_constant; the lambda's
// body is compiled once per value of the picker's list, so THE LIST AT THE CALL SITE IS THE LIST OF INSTANTIATIONS.  The pickers
// return whether a value matched; what a miss returns (QT_ERR_BAD_DTYPE or QT_ERR_BAD_ARG) is the caller's to say.  The folds are left
// folds: hipcc then instantiates the lambda in list order, and the kernels keep that order in the code object.
#pragma once
#include <type_traits>

#include "qt_device.h"

template <int V>
using qt_int = std::integral_constant<int, V>;

// qt_pick<1, 2, 3, 4>(nstage, [&](auto NS) { kernel<decltype(NS)::value><<<...>>>(...); })
template <int... Vs, class F>
inline bool qt_pick(int v, F &&f) {
    return (... || (v == Vs ? (f(qt_int<Vs>{}), true) : false));
}

// qt_pick_bool(amax != nullptr, [&](auto OBS) { kernel<decltype(OBS)::value><<<...>>>(...); })
template <class F>
inline void qt_pick_bool(bool b, F &&f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}

// The Rounder<KIND> argument of a format: a table format whose map carries the row form (p1 bit 0) is kFmtRows.
inline int qt_rounder_kind(const qt_format &fmt) {
    if (fmt.kind == QT_FMT_LUT) return (fmt.p1 & 1) ? kFmtRows : QT_FMT_LUT;
    return fmt.kind == kFmtRows ? -1 : fmt.kind;          // kFmtRows is no kind of the ABI
}

// Rows or table: qt_pick_kind<kFmtRows, QT_FMT_LUT, QT_FMT_FP_SAT, QT_FMT_INT, QT_FMT_IDENTITY>(*fmt, [&](auto K) { ... <decltype(K)::value> ... })
template <int... Kinds, class F>
inline bool qt_pick_kind(const qt_format &fmt, F &&f) {
    return qt_pick<Kinds...>(qt_rounder_kind(fmt), f);
}

// Rows only: a table format is taken only with its table pointer and in the row form, so QT_FMT_LUT is not among Kinds.
template <int... Kinds, class F>
inline bool qt_pick_kind_rows(const qt_format &fmt, const uint16_t *lut, F &&f) {
    static_assert(((Kinds != QT_FMT_LUT) && ...), "rows only: list kFmtRows, not QT_FMT_LUT");
    if (fmt.kind == QT_FMT_LUT && !lut) return false;
    return qt_pick_kind<Kinds...>(fmt, f);
}

// An (a, b) pair out of a fixed list: qt_pick_pair(MxPairs{}, fa, fb, [&](auto P) { kernel<decltype(P)::a, decltype(P)::b><<<...>>>(...); })
template <int A, int B>
struct qt_pair {
    static constexpr int a = A, b = B;
};
template <class... Ps>
struct qt_pairs {};
template <class... Ps, class F>
inline bool qt_pick_pair(qt_pairs<Ps...>, int a, int b, F &&f) {
    return (... || (a == Ps::a && b == Ps::b ? (f(Ps{}), true) : false));
}
