// instance_lists.hpp — compile-time lists of template arguments and the helpers that walk them.  Plain C++, included
// inside the unit's namespace (render_route.hpp and resample_route.hpp include it; the unit includes <type_traits> in
// front).  A launcher dispatches over a list, the instance listing (iamf_route.hip) walks the same list, so the two
// cannot name different instances.
#pragma once

template <int... V>
struct Ints {
  static constexpr bool has(int v) { return ((v == V) || ...); }
};
// Calls f(std::integral_constant<int, V>) for the V of the list that equals v; false if v is not in the list.  (An f that
// returns a value — a dispatch over a second list — decides the result itself.)
template <int V, class F>
bool dispatch_hit(F &f) {
  if constexpr (std::is_void_v<decltype(f(std::integral_constant<int, V>{}))>) {
    f(std::integral_constant<int, V>{});
    return true;
  } else {
    return f(std::integral_constant<int, V>{});
  }
}
template <int... V, class F>
bool dispatch(Ints<V...>, int v, F &&f) {
  return ((v == V && dispatch_hit<V>(f)) || ...);
}
// an (inputs, outputs) pair as one list entry
constexpr int mc(int m, int c) { return m * 32 + c; }
constexpr int mc_m(int v) { return v / 32; }
constexpr int mc_c(int v) { return v % 32; }
// f(v) for every v of the list, in list order
template <int... V, class F>
void for_each_int(Ints<V...>, F &&f) {
  (f(V), ...);
}
