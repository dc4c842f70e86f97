// Host-only: run-time values -> template arguments.  A launcher writes each kernel template's launch once, in a generic lambda whose
// parameters are tags (std::integral_constant / std::bool_constant), and selects the tags with
//     dispatch([&](auto MO, auto PRE) { hipLaunchKernelGGL((kernel<MO(), PRE()>), ...); return BBDM_OK; }, one_of<2, 4, 6>(m), pre != nullptr);
// Only the listed values are instantiated: a launcher whose combinations are not a full product splits them over its branches (or an
// `if constexpr` in the lambda), so that no kernel instance appears that the branches cannot reach.
#pragma once
#include <type_traits>
#include "common.h"

template <int V> using int_tag = std::integral_constant<int, V>;
template <int V> constexpr int_tag<V> int_c{};
constexpr std::true_type yes_tag{};
constexpr std::false_type no_tag{};

template <int... Vs> struct OneOf { int v; };
template <int... Vs> inline OneOf<Vs...> one_of(int v) { return {v}; }

// dispatch(f, selectors...): every selector is a bool or a one_of<...>(int); calls f(tag, tag, ...) once and returns its int.
// A value outside a one_of list is an error (the callers' argument checks make it unreachable), never a silent default.
template <class F> inline int dispatch(F&& f) { return f(); }
template <class F, class... Rest> inline int dispatch(F&& f, bool sel, Rest... rest);
template <class F, int... Vs, class... Rest> inline int dispatch(F&& f, OneOf<Vs...> sel, Rest... rest) {
    int rc = BBDM_E_BADARG;
    const bool hit = ((sel.v == Vs && ((rc = dispatch([&](auto... t) { return f(int_tag<Vs>{}, t...); }, rest...)), true)) || ...);
    if (!hit) bbdm_set_error("dispatch: %d is not among the instantiated values", sel.v);
    return rc;
}
template <class F, class... Rest> inline int dispatch(F&& f, bool sel, Rest... rest) {
    return sel ? dispatch([&](auto... t) { return f(yes_tag, t...); }, rest...)
               : dispatch([&](auto... t) { return f(no_tag, t...); }, rest...);
}
