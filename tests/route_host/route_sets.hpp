// What the per-form checks beside this file share about the row sets behind the listing (for_each_instance_of_set,
// iac_amd/csrc/render_route.hpp).  Included inside the check's namespace, behind render_route.hpp.
//
// The pins are by set NUMBER: a set keeps its number, its row count and its family for good (iamf_hip_route_count goes by the
// number, the family listings by the family), and a form added later is one more set behind these — kRouteSets grows, this table
// and the checks that use it stay as they are.
#pragma once

constexpr int kPinnedSets = 13;
constexpr int kPinnedRows[kPinnedSets] = {408, 9, 16, 20, 36, 4, 18, 20, 36, 36, 72, 18, 36};
// the one family of each set behind the base table (set 0 holds families 1 .. 23)
constexpr int kPinnedFamily[kPinnedSets] = {0, 15, 16, 17, 25, 27, 29, 31, 33, 37, 39, 43, 47};
static_assert(kRouteSets >= kPinnedSets && kRouteTables == 3, "sets are added behind the pinned ones; three numbered tables");

// rows of set `set`, and how many of them are of `family`
inline int rows_of_set(int set, int family = -1, int *of_family = nullptr) {
  int n = 0, nf = 0;
  for_each_instance_of_set(set, [&](int f, int, int, int, int) { ++n, nf += f == family ? 1 : 0; });
  if (of_family) *of_family = nf;
  return n;
}
// every pinned set has its row count and its family — the base table families 1 .. 23, every other set its one family
inline bool pinned_sets_ok() {
  bool ok = true;
  for (int s = 0; s < kPinnedSets; ++s) {
    int n = 0, own = 0;
    for_each_instance_of_set(s, [&](int f, int, int, int, int) { ++n, own += (s == 0 ? f >= 1 && f <= 23 : f == kPinnedFamily[s]) ? 1 : 0; });
    ok = ok && n == kPinnedRows[s] && own == n;
  }
  return ok;
}
// no row for a set number outside the listing
inline bool no_rows_outside() { return rows_of_set(-1) == 0 && rows_of_set(kRouteSets) == 0; }
// `family` is the one family of set `set`, with `rows` rows, and appears in no other set of the listing
inline bool family_in_one_set(int family, int set, int rows) {
  bool ok = true;
  for (int s = 0; s < kRouteSets; ++s) {
    int of_family = 0;
    const int n = rows_of_set(s, family, &of_family);
    ok = ok && (s == set ? n == rows && of_family == rows : of_family == 0);
  }
  return ok;
}
// the sets that list a key, as a mask over every set of the listing
inline int sets_of_key(int family, int variant, int m, int c, int k) {
  int mask = 0;
  for (int s = 0; s < kRouteSets; ++s)
    for_each_instance_of_set(s, [&](int f, int v, int km, int kc, int kk) { mask |= (f == family && v == variant && km == m && kc == c && kk == k) ? 1 << s : 0; });
  return mask;
}
