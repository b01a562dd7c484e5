// Storage, key lookup and validation of the tuning knobs -- everything generated from the one table in cfen_tune_knobs.hpp.
// Host only: nothing here touches the GPU.
#include <initializer_list>
#include <stdio.h>
#include <string.h>

#include "../../include/cfen_hip.h"
#include "cfen_common.hpp"

namespace {

struct Rule {
  enum Kind { ANY, ON_OFF, LOW_BITS, RANGE, AT_LEAST, ONE_OF } kind;
  int lo, hi;
  int nset, set[16];
};
constexpr Rule any_int() { return {Rule::ANY, 0, 0, 0, {}}; }
constexpr Rule on_off() { return {Rule::ON_OFF, 0, 0, 0, {}}; }
constexpr Rule low_bits(int mask) { return {Rule::LOW_BITS, mask, 0, 0, {}}; }
constexpr Rule range(int lo, int hi) { return {Rule::RANGE, lo, hi, 0, {}}; }
constexpr Rule at_least(int lo) { return {Rule::AT_LEAST, lo, 0, 0, {}}; }
constexpr Rule one_of(std::initializer_list<int> values) {
  Rule r = {Rule::ONE_OF, 0, 0, 0, {}};
  for (int v : values) r.set[r.nset++] = v;   // more than 16 values do not compile: the table is constexpr
  return r;
}

enum {
#define CFEN_KNOB(ident, key, shipped, rule) K_##ident,
#include "cfen_tune_knobs.hpp"
#undef CFEN_KNOB
  N_KNOBS
};

struct Knob { const char* key; int shipped; Rule rule; };
constexpr Knob g_knob[N_KNOBS] = {
#define CFEN_KNOB(ident, key, shipped, rule) {key, shipped, rule},
#include "cfen_tune_knobs.hpp"
#undef CFEN_KNOB
};

int g_value[N_KNOBS] = {
#define CFEN_KNOB(ident, key, shipped, rule) shipped,
#include "cfen_tune_knobs.hpp"
#undef CFEN_KNOB
};

int find(const char* key) {
  for (int k = 0; k < N_KNOBS; ++k)
    if (!strcmp(key, g_knob[k].key)) return k;
  return -1;
}

}  // namespace

#define CFEN_KNOB(ident, key, shipped, rule) int& cfen_tune_##ident() { return g_value[K_##ident]; }
#include "cfen_tune_knobs.hpp"
#undef CFEN_KNOB

int cfen_tune(const char* key, int value) {
  CFEN_CHECK_ARG(key != nullptr, "tune: null key");
  const int k = find(key);
  CFEN_CHECK_ARG(k >= 0, "tune: unknown key '%s'", key);
  const Rule& r = g_knob[k].rule;
  switch (r.kind) {
    case Rule::ANY: break;
    case Rule::ON_OFF: value = value != 0; break;
    case Rule::LOW_BITS: value &= r.lo; break;
    case Rule::RANGE: CFEN_CHECK_ARG(value >= r.lo && value <= r.hi, "tune: %s must be %d .. %d, got %d", key, r.lo, r.hi, value); break;
    case Rule::AT_LEAST: CFEN_CHECK_ARG(value >= r.lo, "tune: %s must be >= %d, got %d", key, r.lo, value); break;
    case Rule::ONE_OF: {
      bool ok = false;
      char takes[128] = "";
      for (int i = 0, n = 0; i < r.nset; ++i) {
        ok |= r.set[i] == value;
        n += snprintf(takes + n, sizeof(takes) - n, i ? ", %d" : "%d", r.set[i]);
      }
      CFEN_CHECK_ARG(ok, "tune: %s must be one of %s, got %d", key, takes, value);
      break;
    }
  }
  g_value[k] = value;
  return CFEN_OK;
}

int cfen_tune_query(const char* key, int* value, int* shipped_default) {
  CFEN_CHECK_ARG(key != nullptr, "tune_query: null key");
  const int k = find(key);
  CFEN_CHECK_ARG(k >= 0, "tune_query: unknown key '%s'", key);
  if (value) *value = g_value[k];
  if (shipped_default) *shipped_default = g_knob[k].shipped;
  return CFEN_OK;
}

const char* cfen_tune_key(int index) { return index >= 0 && index < N_KNOBS ? g_knob[index].key : nullptr; }
