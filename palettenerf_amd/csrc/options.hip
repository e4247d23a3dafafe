// options.hip -- the run-time switches' storage (g_opt_<name>, initialised from the environment when the library is loaded) and pnr_set_option.
// Everything about a switch is its line of options.def; the rules are options.hpp's.  No kernel lives here.
#include "../../include/pnr.h"
#include "options.hpp"

static const char* env_lookup(const char* var) { return getenv(var); }
static int* const g_slots[] = {
#define PNR_OPTION(name, def, set, env, what) &g_opt_##name,
#define PNR_FRAME_OPTION PNR_OPTION
#include "options.def"
};
#define PNR_OPTION(name, def, set, env, what) int g_opt_##name = pnr::option_initial(pnr::kOptions[pnr::option_index(#name)], env_lookup);
#define PNR_FRAME_OPTION PNR_OPTION
#include "options.def"

extern "C" int pnr_set_option(const char* name, int value) {
    const int i = pnr::option_index(name);
    if (i < 0) return PNR_ERR_INVALID;
    *g_slots[i] = pnr::option_stored(pnr::kOptions[i], value);
    return PNR_OK;
}
