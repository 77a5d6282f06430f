// iamf_route.hip — which kernel ran (include/iamf_hip.h: iamf_hip_route_instances, iamf_hip_route_tally and their indexed and
// per-family forms).  Host code only.  One array of row sets, each built by walking the lists the launchers dispatch over
// (for_each_instance_of_set, render_route.hpp), so a kernel instance added to a list — or a set added to that walker — is
// listed and counted without a change here.  Every launcher counts through the one entry iamf_hip_route_count(set, ..), the
// set being RouteKey::set of the route it ran.  Counting is one relaxed atomic add per launch on a fixed array: no lock and no
// allocation on the call path (the decoder groups launch from several threads).
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <type_traits>

#include "../../include/iamf_hip.h"
#include "render_entry.hpp"

namespace {

#include "render_params.hpp"
#include "render_route.hpp"

constexpr int kRouteCap = 1024;   // rows the table can hold; slot kRouteCap counts launches outside the table

constexpr uint32_t pack_key(int family, int variant, int m, int c, int k) {
  return (uint32_t)family << 24 | (uint32_t)variant << 20 | (uint32_t)m << 12 | (uint32_t)c << 4 | (uint32_t)k;
}

struct RouteTable {
  iamf_hip_route_row rows[kRouteCap];
  uint32_t key[kRouteCap];     // sorted
  int32_t index[kRouteCap];    // row of key[i]
  int n = 0, dropped = 0;
  void build(int set) {
    const auto add = [&](int family, int variant, int m, int c, int k) {
      if (n == kRouteCap) {
        ++dropped;
        return;
      }
      iamf_hip_route_row &r = rows[n];
      memset(&r, 0, sizeof(r));
      r.family = family;
      r.variant = variant;
      r.m = m;
      r.c = c;
      r.k = k;
      key[n] = pack_key(family, variant, m, c, k);
      index[n] = n;
      ++n;
    };
    if (set < kRouteSets) for_each_instance_of_set(set, add);
    else for_each_instance_of_later_set(set - kRouteSets, add);   // (the sets behind: render_route.hpp)
    int32_t order[kRouteCap];
    for (int i = 0; i < n; ++i) order[i] = i;
    std::sort(order, order + n, [&](int a, int b) { return key[a] < key[b]; });
    uint32_t sorted[kRouteCap];
    for (int i = 0; i < n; ++i) sorted[i] = key[order[i]];
    memcpy(key, sorted, sizeof(uint32_t) * n);
    memcpy(index, order, sizeof(int32_t) * n);
  }
  int find(uint32_t k) const {
    const uint32_t *e = key + n, *p = std::lower_bound(key, e, k);
    return (p != e && *p == k) ? index[p - key] : kRouteCap;
  }
};

// One row set and its counters (slot kRouteCap: IAMF_HIP_ROUTE_NONE).  Sets 0 .. kRouteTables - 1 ARE the numbered tables
// of iamf_hip_route_table_instances (0: the base listing, 1: the extension, 2: the 24-bit LPCM form), whose count is pinned;
// the sets behind them are listed by family only (iamf_hip_route_family_instances).  for_each_instance_of_set
// (render_route.hpp) says which rows fill which of the kRouteSets sets, for_each_instance_of_later_set which fill the
// kRouteLaterSets sets behind them (also listed by family only).
constexpr int kRouteSetsAll = kRouteSets + kRouteLaterSets;
struct RouteSet {
  RouteTable table;
  std::atomic<int64_t> launches[kRouteCap + 1];
};
RouteSet *route_sets() {
  static RouteSet *const sets = [] {
    static RouteSet s[kRouteSetsAll];   // (static storage: every counter starts at zero)
    for (int set = 0; set < kRouteSetsAll; ++set) s[set].table.build(set);
    return s;
  }();
  return sets;
}
RouteSet *numbered_table(int table) { return table >= 0 && table < kRouteTables ? &route_sets()[table] : nullptr; }

int list_instances(const RouteTable &t, iamf_hip_route_row *rows, int cap) {
  for (int i = 0; rows && i < t.n && i < cap; ++i) rows[i] = t.rows[i];
  return t.n + t.dropped;
}

int tally_of(RouteSet &s, iamf_hip_route_row *rows, int cap, int reset) {
  const RouteTable &t = s.table;
  int cnt = 0;
  for (int i = 0; i <= kRouteCap; ++i) {
    if (i >= t.n && i != kRouteCap) continue;
    const int64_t v = reset ? s.launches[i].exchange(0, std::memory_order_relaxed) : s.launches[i].load(std::memory_order_relaxed);
    if (v == 0) continue;
    if (rows && cnt < cap) {
      if (i < t.n) rows[cnt] = t.rows[i];
      else memset(&rows[cnt], 0, sizeof(rows[cnt]));   // IAMF_HIP_ROUTE_NONE
      rows[cnt].launches = v;
    }
    ++cnt;
  }
  return cnt;
}

// the rows of one family, in the order of their sets.  tally: only rows whose counter is not zero, with its value (reset:
// and zeroed); else the listing.  -1: no set has a row of that family
int family_rows(int family, bool tally, iamf_hip_route_row *rows, int cap, int reset) {
  int cnt = 0;
  bool known = false;
  for (int set = 0; set < kRouteSetsAll; ++set) {
    RouteSet &s = route_sets()[set];
    const RouteTable &t = s.table;
    for (int i = 0; i < t.n; ++i) {
      if (t.rows[i].family != family) continue;
      known = true;
      int64_t v = 0;
      if (tally) {
        v = reset ? s.launches[i].exchange(0, std::memory_order_relaxed) : s.launches[i].load(std::memory_order_relaxed);
        if (v == 0) continue;
      }
      if (rows && cnt < cap) {
        rows[cnt] = t.rows[i];
        rows[cnt].launches = v;
      }
      ++cnt;
    }
  }
  return known ? cnt : -1;
}

}  // namespace

// A key its set does not hold counts in that set's own NONE slot where the set is a numbered table, else (the sets listed by
// family only have no tally of their own to show it) in the base table's.
void iamf_hip_route_count(int set, int family, int variant, int m, int c, int k) {
  if (set < 0 || set >= kRouteSetsAll) return;
  RouteSet *sets = route_sets();
  const int i = sets[set].table.find(pack_key(family, variant, m, c, k));
  sets[i == kRouteCap && set >= kRouteTables ? 0 : set].launches[i].fetch_add(1, std::memory_order_relaxed);
}

extern "C" {

int iamf_hip_route_tables(void) { return kRouteTables; }

int iamf_hip_route_table_instances(int table, iamf_hip_route_row *rows, int cap) {
  const RouteSet *s = numbered_table(table);
  return s ? list_instances(s->table, rows, cap) : IAMF_HIP_ERR_BAD_ARG;
}

int iamf_hip_route_table_tally(int table, iamf_hip_route_row *rows, int cap, int reset) {
  RouteSet *s = numbered_table(table);
  return s ? tally_of(*s, rows, cap, reset) : IAMF_HIP_ERR_BAD_ARG;
}

int iamf_hip_route_family_instances(int family, iamf_hip_route_row *rows, int cap) {
  return family_rows(family, false, rows, cap, 0);
}

int iamf_hip_route_family_tally(int family, iamf_hip_route_row *rows, int cap, int reset) {
  return family_rows(family, true, rows, cap, reset);
}

int iamf_hip_route_instances(iamf_hip_route_row *rows, int cap) { return iamf_hip_route_table_instances(0, rows, cap); }

int iamf_hip_route_tally(iamf_hip_route_row *rows, int cap, int reset) { return iamf_hip_route_table_tally(0, rows, cap, reset); }

int iamf_hip_route_instances_ext(iamf_hip_route_row *rows, int cap) { return iamf_hip_route_table_instances(1, rows, cap); }

int iamf_hip_route_tally_ext(iamf_hip_route_row *rows, int cap, int reset) { return iamf_hip_route_table_tally(1, rows, cap, reset); }

}  // extern "C"
