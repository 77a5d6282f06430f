// iamf_route.hip — which kernel ran (include/iamf_hip.h: iamf_hip_route_instances, iamf_hip_route_tally).  Host code only.
// The table is built by walking the lists the launchers dispatch over (render_route.hpp, resample_route.hpp), so a kernel
// instance added to a list is listed and counted without a change here.  Counting is one relaxed atomic add per launch on a
// fixed array: no lock and no allocation on the call path (the decoder groups launch from several threads).
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
#include "resample_route.hpp"

constexpr int kRouteCap = 1024;   // rows the table can hold; slot kRouteCap counts launches outside the table

constexpr uint32_t pack_key(int family, int variant, int m, int c, int k) {
  return (uint32_t)family << 24 | (uint32_t)variant << 20 | (uint32_t)m << 12 | (uint32_t)c << 4 | (uint32_t)k;
}

struct RouteTable {
  iamf_hip_route_row rows[kRouteCap];
  uint32_t key[kRouteCap];     // sorted
  int32_t index[kRouteCap];    // row of key[i]
  int n = 0, dropped = 0;
  explicit RouteTable(int table) {
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
    if (table == 5) {
      for_each_render_instance_interleaved(add);
    } else if (table == 4) {
      for_each_render_instance_lpcm_mix(add);
    } else if (table == 3) {
      for_each_render_instance_lpcm_coupled(add);
    } else if (table == 2) {
      for_each_render_instance_lpcm24(add);
    } else if (table == 1) {
      for_each_render_instance_ext(add);
    } else {
      for_each_render_instance(add);
      for_each_resample_instance(add);
    }
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

const RouteTable &route_table() {
  static const RouteTable t(0);
  return t;
}

// the extension table: the same row type and semantics, its own rows and its own counters (iamf_hip_route_instances_ext)
const RouteTable &route_table_ext() {
  static const RouteTable t(1);
  return t;
}

// table 2: the 24-bit LPCM form (iamf_hip_route_table_instances)
const RouteTable &route_table_lpcm24() {
  static const RouteTable t(2);
  return t;
}

// behind the numbered tables: the coupled 16-bit LPCM form, listed per family only (iamf_hip_route_family_instances)
const RouteTable &route_table_lpcm_coupled() {
  static const RouteTable t(3);
  return t;
}

// ... and the two-element packet form (LPCM_MIX), likewise
const RouteTable &route_table_lpcm_mix() {
  static const RouteTable t(4);
  return t;
}

// ... and the interleaved f32 form (FAST_INTERLEAVED)
const RouteTable &route_table_interleaved() {
  static const RouteTable t(5);
  return t;
}

std::atomic<int64_t> g_launches[kRouteCap + 1];
std::atomic<int64_t> g_launches_ext[kRouteCap + 1];
std::atomic<int64_t> g_launches_lpcm24[kRouteCap + 1];
std::atomic<int64_t> g_launches_lpcm_coupled[kRouteCap + 1];
std::atomic<int64_t> g_launches_lpcm_mix[kRouteCap + 1];
std::atomic<int64_t> g_launches_interleaved[kRouteCap + 1];

// the indexed form: table 0 and 1 ARE the base and the extension listing (rows and counters), 2 onwards have their own
constexpr int kRouteTables = 3;
const RouteTable *table_of(int table) {
  return table == 0 ? &route_table() : table == 1 ? &route_table_ext() : table == 2 ? &route_table_lpcm24() : nullptr;
}
std::atomic<int64_t> *launches_of(int table) {
  return table == 0 ? g_launches : table == 1 ? g_launches_ext : table == 2 ? g_launches_lpcm24 : nullptr;
}
// The listing by family (iamf_hip_route_family_instances) walks every row set there is: the numbered tables, whose count is
// pinned, and the sets added since, which have no number.  A family added to a set — or a set added here — is listed
// without a new entry point.
constexpr int kRouteSets = 6;
const RouteTable *set_of(int set) {
  return set < kRouteTables ? table_of(set)
         : set == 3 ? &route_table_lpcm_coupled()
         : set == 4 ? &route_table_lpcm_mix()
         : set == 5 ? &route_table_interleaved()
                    : nullptr;
}
std::atomic<int64_t> *set_launches_of(int set) {
  return set < kRouteTables ? launches_of(set)
         : set == 3 ? g_launches_lpcm_coupled
         : set == 4 ? g_launches_lpcm_mix
         : set == 5 ? g_launches_interleaved
                    : nullptr;
}

int list_instances(const RouteTable &t, iamf_hip_route_row *rows, int cap) {
  for (int i = 0; rows && i < t.n && i < cap; ++i) rows[i] = t.rows[i];
  return t.n + t.dropped;
}

int tally_of(const RouteTable &t, std::atomic<int64_t> *launches, iamf_hip_route_row *rows, int cap, int reset) {
  int cnt = 0;
  for (int i = 0; i <= kRouteCap; ++i) {
    if (i >= t.n && i != kRouteCap) continue;
    const int64_t v = reset ? launches[i].exchange(0, std::memory_order_relaxed) : launches[i].load(std::memory_order_relaxed);
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
  for (int set = 0; set < kRouteSets; ++set) {
    const RouteTable &t = *set_of(set);
    std::atomic<int64_t> *launches = set_launches_of(set);
    for (int i = 0; i < t.n; ++i) {
      if (t.rows[i].family != family) continue;
      known = true;
      int64_t v = 0;
      if (tally) {
        v = reset ? launches[i].exchange(0, std::memory_order_relaxed) : launches[i].load(std::memory_order_relaxed);
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

void iamf_hip_route_count_family(int family, int variant, int m, int c, int k) {
  const uint32_t key = pack_key(family, variant, m, c, k);
  for (int set = 0; set < kRouteSets; ++set) {
    const int i = set_of(set)->find(key);
    if (i == kRouteCap) continue;
    set_launches_of(set)[i].fetch_add(1, std::memory_order_relaxed);
    return;
  }
  g_launches[kRouteCap].fetch_add(1, std::memory_order_relaxed);   // outside every set: the base tally's NONE row
}

void iamf_hip_route_count(int family, int variant, int m, int c, int k) {
  g_launches[route_table().find(pack_key(family, variant, m, c, k))].fetch_add(1, std::memory_order_relaxed);
}

void iamf_hip_route_count_ext(int family, int variant, int m, int c, int k) {
  g_launches_ext[route_table_ext().find(pack_key(family, variant, m, c, k))].fetch_add(1, std::memory_order_relaxed);
}

void iamf_hip_route_count_table(int table, int family, int variant, int m, int c, int k) {
  const RouteTable *t = table_of(table);
  if (t) launches_of(table)[t->find(pack_key(family, variant, m, c, k))].fetch_add(1, std::memory_order_relaxed);
}

extern "C" {

int iamf_hip_route_tables(void) { return kRouteTables; }

int iamf_hip_route_table_instances(int table, iamf_hip_route_row *rows, int cap) {
  const RouteTable *t = table_of(table);
  return t ? list_instances(*t, rows, cap) : IAMF_HIP_ERR_BAD_ARG;
}

int iamf_hip_route_table_tally(int table, iamf_hip_route_row *rows, int cap, int reset) {
  const RouteTable *t = table_of(table);
  return t ? tally_of(*t, launches_of(table), rows, cap, reset) : IAMF_HIP_ERR_BAD_ARG;
}

int iamf_hip_route_family_instances(int family, iamf_hip_route_row *rows, int cap) {
  return family_rows(family, false, rows, cap, 0);
}

int iamf_hip_route_family_tally(int family, iamf_hip_route_row *rows, int cap, int reset) {
  return family_rows(family, true, rows, cap, reset);
}

int iamf_hip_route_instances(iamf_hip_route_row *rows, int cap) { return list_instances(route_table(), rows, cap); }

int iamf_hip_route_tally(iamf_hip_route_row *rows, int cap, int reset) {
  return tally_of(route_table(), g_launches, rows, cap, reset);
}

int iamf_hip_route_instances_ext(iamf_hip_route_row *rows, int cap) { return list_instances(route_table_ext(), rows, cap); }

int iamf_hip_route_tally_ext(iamf_hip_route_row *rows, int cap, int reset) {
  return tally_of(route_table_ext(), g_launches_ext, rows, cap, reset);
}

}  // extern "C"
