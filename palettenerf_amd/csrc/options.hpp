// options.hpp -- the run-time switches of pnr_set_option as one table (options.def): their `extern int g_opt_<name>` declarations, what a set stores,
// and the value a process starts with.  Host only, no HIP dependencies, so that tests/native/ can compile it with g++ and compare it with the chain of
// comparisons and the getenv initialisers it replaced (options_check.cpp).  The definitions and pnr_set_option itself are in options.hip.
#pragma once
#include <stdlib.h>
#include <string.h>

#define PNR_OPTION(name, def, set, env, what) extern int g_opt_##name;
#define PNR_FRAME_OPTION PNR_OPTION
#include "options.def"

namespace pnr {

struct SetRule { enum Kind { kBool, kClamp, kMin, kMask } kind; int lo, hi; };
constexpr SetRule set_bool() { return {SetRule::kBool, 0, 0}; }
constexpr SetRule set_clamp(int lo, int hi) { return {SetRule::kClamp, lo, hi}; }
constexpr SetRule set_min(int lo) { return {SetRule::kMin, lo, 0}; }
constexpr SetRule set_mask(int m) { return {SetRule::kMask, m, 0}; }

// checked in this order: `off` set -> 0, `on` set -> 1, `value` set -> atoi of it (as_flag: != 0); none set -> the default
struct EnvRule { const char *off, *on, *value; bool as_flag; };
constexpr EnvRule env_none() { return {nullptr, nullptr, nullptr, false}; }
constexpr EnvRule env_off(const char* var) { return {var, nullptr, nullptr, false}; }
constexpr EnvRule env_on(const char* var) { return {nullptr, var, nullptr, false}; }
constexpr EnvRule env_int(const char* var) { return {nullptr, nullptr, var, false}; }
constexpr EnvRule env_flag(const char* var) { return {nullptr, nullptr, var, true}; }
constexpr EnvRule env_off_or_int(const char* no_var, const char* var) { return {no_var, nullptr, var, false}; }

struct Option { const char* name; int def; SetRule set; EnvRule env; bool per_frame; const char* what; };
constexpr Option kOptions[] = {
#define PNR_OPTION(name, def, set, env, what) {#name, def, set, env, false, what},
#define PNR_FRAME_OPTION(name, def, set, env, what) {#name, def, set, env, true, what},
#include "options.def"
};
constexpr int kNumOptions = (int)(sizeof(kOptions) / sizeof(kOptions[0]));

// index into kOptions, -1 for a name the table does not hold (or none)
inline int option_index(const char* name) {
    if (!name) return -1;
    for (int i = 0; i < kNumOptions; i++)
        if (!strcmp(name, kOptions[i].name)) return i;
    return -1;
}
// what pnr_set_option(o.name, value) stores
inline int option_stored(const Option& o, int value) {
    switch (o.set.kind) {
        case SetRule::kBool: return value != 0;
        case SetRule::kClamp: return value < o.set.lo ? o.set.lo : (value > o.set.hi ? o.set.hi : value);
        case SetRule::kMin: return value < o.set.lo ? o.set.lo : value;
        default: return value & o.set.lo;
    }
}
// the value a process starts with; lookup = getenv, or a test's stand-in
inline int option_initial(const Option& o, const char* (*lookup)(const char*)) {
    if (o.env.off && lookup(o.env.off)) return 0;
    if (o.env.on && lookup(o.env.on)) return 1;
    if (const char* v = o.env.value ? lookup(o.env.value) : nullptr) return o.env.as_flag ? atoi(v) != 0 : atoi(v);
    return o.def;
}

}  // namespace pnr
