// options_check.cpp -- csrc/options.hpp (the table of options.def and its rules) against what it replaced: pnr_set_option's chain of comparisons and the
// getenv initialisers, transcribed below as they stood at the bottom of raymarch.hip.  Stand-alone: exit status 0 when every case agrees, 1 (and the
// first mismatch on stderr) otherwise.  The environment is a stand-in (a lookup over a small list), never the process's own.
#include "../../palettenerf_amd/csrc/options.hpp"
#include "../../include/pnr.h"
#include <initializer_list>
#include <limits.h>
#include <stdio.h>

// the stand-in environment: up to two variables
static const char *g_var[2], *g_val[2];
static const char* fake_env(const char* name) {
    for (int i = 0; i < 2; i++)
        if (g_var[i] && !strcmp(g_var[i], name)) return g_val[i];
    return nullptr;
}

namespace old {
#define getenv fake_env
struct Opts {
    int g_opt_block_skip = getenv("PNR_NO_BLOCK_SKIP") ? 0 : 1;
    int g_opt_coop_march = getenv("PNR_NO_COOP_MARCH") ? 0 : 1;
    int g_opt_hosted_tail = getenv("PNR_NO_HOSTED_TAIL") ? 0 : 1;
    int g_opt_march_budget = getenv("PNR_MARCH_BUDGET") ? atoi(getenv("PNR_MARCH_BUDGET")) : 2;
    int g_opt_march_budget0 = getenv("PNR_MARCH_BUDGET0") ? atoi(getenv("PNR_MARCH_BUDGET0")) : 0;
    int g_opt_march_blocks = getenv("PNR_MARCH_BLOCKS") ? atoi(getenv("PNR_MARCH_BLOCKS")) : 0;
    int g_opt_aux_fusion = getenv("PNR_NO_AUX_FUSION") ? 0 : 1;
    int g_opt_composite_fusion = getenv("PNR_NO_COMPOSITE_FUSION") ? 0 : (getenv("PNR_COMPOSITE_FUSION") ? atoi(getenv("PNR_COMPOSITE_FUSION")) : 2);
    int g_opt_iteration_margin = getenv("PNR_ITERATION_MARGIN") ? atoi(getenv("PNR_ITERATION_MARGIN")) : 0;
    int g_opt_palette_waves12 = getenv("PNR_PALETTE_WAVES8") ? 0 : 1;
    int g_opt_dynamic_tiles = getenv("PNR_DYNAMIC_TILES") ? 1 : 0;
    int g_opt_grid_lane_pairs = getenv("PNR_GRID_LANE_PAIRS") ? atoi(getenv("PNR_GRID_LANE_PAIRS")) != 0 : 1;
    int g_opt_grid_fast = getenv("PNR_NO_GRID_FAST") ? 0 : 1;
    int g_opt_train_coop = getenv("PNR_NO_TRAIN_COOP") ? 0 : 1;
    int g_opt_mlp_f16x3 = getenv("PNR_MLP_FP32") ? 0 : 1;
    int g_opt_coarse_image = getenv("PNR_NO_COARSE_IMAGE") ? 0 : 1;
    int g_opt_scatter_staged = getenv("PNR_NO_SCATTER_STAGED") ? 0 : 1;
    int g_opt_cell_merge = getenv("PNR_NO_CELL_MERGE") ? 0 : 1;
    int g_opt_flex_coop = getenv("PNR_NO_FLEX_COOP") ? 0 : 1;
    int g_opt_grid_nt = getenv("PNR_GRID_NT") ? atoi(getenv("PNR_GRID_NT")) : 0;
    int g_opt_adam_variant = 0;

    int pnr_set_option(const char* name, int value) {
        if (!name) return PNR_ERR_INVALID;
        if (!strcmp(name, "block_skip")) { g_opt_block_skip = value != 0; return PNR_OK; }
        if (!strcmp(name, "coop_march")) { g_opt_coop_march = value != 0; return PNR_OK; }
        if (!strcmp(name, "hosted_tail")) { g_opt_hosted_tail = value != 0; return PNR_OK; }
        if (!strcmp(name, "march_budget")) { g_opt_march_budget = value < 1 ? 1 : (value > 1024 ? 1024 : value); return PNR_OK; }
        if (!strcmp(name, "march_budget0")) { g_opt_march_budget0 = value < 0 ? 0 : (value > 1024 ? 1024 : value); return PNR_OK; }
        if (!strcmp(name, "march_blocks")) { g_opt_march_blocks = value < 0 ? 0 : value; return PNR_OK; }
        if (!strcmp(name, "aux_fusion")) { g_opt_aux_fusion = value != 0; return PNR_OK; }
        if (!strcmp(name, "composite_fusion")) { g_opt_composite_fusion = value < 0 ? 0 : (value > 2 ? 2 : value); return PNR_OK; }
        if (!strcmp(name, "palette_waves12")) { g_opt_palette_waves12 = value != 0; return PNR_OK; }
        if (!strcmp(name, "dynamic_tiles")) { g_opt_dynamic_tiles = value != 0; return PNR_OK; }
        if (!strcmp(name, "grid_lane_pairs")) { g_opt_grid_lane_pairs = value != 0; return PNR_OK; }
        if (!strcmp(name, "grid_fast")) { g_opt_grid_fast = value != 0; return PNR_OK; }
        if (!strcmp(name, "train_coop")) { g_opt_train_coop = value != 0; return PNR_OK; }
        if (!strcmp(name, "mlp_f16x3")) { g_opt_mlp_f16x3 = value != 0; return PNR_OK; }
        if (!strcmp(name, "coarse_image")) { g_opt_coarse_image = value != 0; return PNR_OK; }
        if (!strcmp(name, "cell_merge")) { g_opt_cell_merge = value != 0; return PNR_OK; }
        if (!strcmp(name, "scatter_staged")) { g_opt_scatter_staged = value != 0; return PNR_OK; }
        if (!strcmp(name, "flex_coop")) { g_opt_flex_coop = value != 0; return PNR_OK; }
        if (!strcmp(name, "grid_nt")) { g_opt_grid_nt = value & 3; return PNR_OK; }
        if (!strcmp(name, "adam_variant")) { g_opt_adam_variant = value & 7; return PNR_OK; }
        if (!strcmp(name, "iteration_margin")) { g_opt_iteration_margin = value < 0 ? 0 : (value > 64 ? 64 : value); return PNR_OK; }
        return PNR_ERR_INVALID;
    }
    // the variable a name stood for (nullptr: none)
    int* slot(const char* name) {
#define SLOT(n) if (!strcmp(name, #n)) return &g_opt_##n;
        SLOT(block_skip) SLOT(coop_march) SLOT(hosted_tail) SLOT(march_budget) SLOT(march_budget0) SLOT(march_blocks) SLOT(aux_fusion)
        SLOT(composite_fusion) SLOT(iteration_margin) SLOT(palette_waves12) SLOT(dynamic_tiles) SLOT(grid_lane_pairs) SLOT(grid_fast) SLOT(train_coop)
        SLOT(mlp_f16x3) SLOT(coarse_image) SLOT(scatter_staged) SLOT(cell_merge) SLOT(flex_coop) SLOT(grid_nt) SLOT(adam_variant)
#undef SLOT
        return nullptr;
    }
};
#undef getenv
constexpr int kNumOptions = 21;   // lines of the chain above
const char* const kEnvVars[] = {"PNR_NO_BLOCK_SKIP", "PNR_NO_COOP_MARCH", "PNR_NO_HOSTED_TAIL", "PNR_MARCH_BUDGET", "PNR_MARCH_BUDGET0", "PNR_MARCH_BLOCKS",
                                "PNR_NO_AUX_FUSION", "PNR_NO_COMPOSITE_FUSION", "PNR_COMPOSITE_FUSION", "PNR_ITERATION_MARGIN", "PNR_PALETTE_WAVES8",
                                "PNR_DYNAMIC_TILES", "PNR_GRID_LANE_PAIRS", "PNR_NO_GRID_FAST", "PNR_NO_TRAIN_COOP", "PNR_MLP_FP32", "PNR_NO_COARSE_IMAGE",
                                "PNR_NO_SCATTER_STAGED", "PNR_NO_CELL_MERGE", "PNR_NO_FLEX_COOP", "PNR_GRID_NT"};
}  // namespace old

// include/pnr.h at pnr_nerf_render_frame_submit: "the pnr_set_option switches _submit saw"
static const char* const kFrameOptions[] = {"aux_fusion", "composite_fusion", "hosted_tail", "march_budget", "march_budget0", "march_blocks",
                                            "iteration_margin", "dynamic_tiles", "block_skip", "coop_march", "palette_waves12", "grid_lane_pairs"};

#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "options_check: " __VA_ARGS__); fprintf(stderr, "\n"); return 1; } } while (0)

// every option's starting value under the stand-in environment as it is now: the table's against the transcription's
static int check_initial(const char* what) {
    old::Opts o;
    for (int i = 0; i < pnr::kNumOptions; i++) {
        const int* want = o.slot(pnr::kOptions[i].name);
        CHECK(want, "%s: the transcription has no option \"%s\"", what, pnr::kOptions[i].name);
        const int got = pnr::option_initial(pnr::kOptions[i], fake_env);
        CHECK(got == *want, "%s: %s starts as %d, expected %d", what, pnr::kOptions[i].name, got, *want);
    }
    return 0;
}

int main() {
    // 3. the table itself
    CHECK(pnr::kNumOptions == old::kNumOptions, "%d options in the table, %d in the chain", pnr::kNumOptions, old::kNumOptions);
    for (int i = 0; i < pnr::kNumOptions; i++)
        for (int j = i + 1; j < pnr::kNumOptions; j++) CHECK(strcmp(pnr::kOptions[i].name, pnr::kOptions[j].name) != 0, "\"%s\" twice", pnr::kOptions[i].name);
    int n_frame = 0;
    for (int i = 0; i < pnr::kNumOptions; i++) {
        bool listed = false;
        for (const char* f : kFrameOptions) listed = listed || !strcmp(f, pnr::kOptions[i].name);
        CHECK(listed == pnr::kOptions[i].per_frame, "\"%s\": per frame %d, listed in pnr.h %d", pnr::kOptions[i].name, (int)pnr::kOptions[i].per_frame, (int)listed);
        n_frame += listed;
    }
    CHECK(n_frame == (int)(sizeof(kFrameOptions) / sizeof(kFrameOptions[0])), "%d of pnr.h's per-frame options are in the table", n_frame);
    for (int i = 0; i < pnr::kNumOptions; i++)
        for (const char* var : {pnr::kOptions[i].env.off, pnr::kOptions[i].env.on, pnr::kOptions[i].env.value}) {
            bool known = !var;
            for (const char* v : old::kEnvVars) known = known || !strcmp(v, var);
            CHECK(known, "\"%s\" reads %s, which nothing read before", pnr::kOptions[i].name, var);
        }

    // 1. pnr_set_option: every name, an unknown one and none; every value of [-3, 1100] and three far ones
    const char* names[old::kNumOptions + 2];
    for (int i = 0; i < pnr::kNumOptions; i++) names[i] = pnr::kOptions[i].name;
    names[old::kNumOptions] = "no_such_option"; names[old::kNumOptions + 1] = nullptr;
    for (const char* name : names) {
        old::Opts o;
        int* want = name ? o.slot(name) : nullptr;
        for (long long v = -3; v <= 1103; v++) {
            const int value = v <= 1100 ? (int)v : (v == 1101 ? INT_MIN : (v == 1102 ? INT_MAX : 65536));
            const int want_rc = o.pnr_set_option(name, value);
            const int i = pnr::option_index(name);
            CHECK((i < 0 ? PNR_ERR_INVALID : PNR_OK) == want_rc, "pnr_set_option(%s, %d): return code", name ? name : "NULL", value);
            if (i >= 0) {
                CHECK(want, "the transcription has no option \"%s\"", name);
                const int got = pnr::option_stored(pnr::kOptions[i], value);
                CHECK(got == *want, "pnr_set_option(%s, %d) stores %d, expected %d", name, value, got, *want);
            }
        }
    }

    // 2. the environment: nothing set; each variable alone with each value; both of composite_fusion's together
    if (check_initial("empty environment")) return 1;
    const char* const values[] = {"", "0", "1", "2", "7", "5000", "-1"};
    for (const char* var : old::kEnvVars)
        for (const char* val : values) {
            g_var[0] = var; g_val[0] = val;
            char what[96];
            snprintf(what, sizeof(what), "%s=\"%s\"", var, val);
            if (check_initial(what)) return 1;
        }
    g_var[0] = "PNR_NO_COMPOSITE_FUSION"; g_var[1] = "PNR_COMPOSITE_FUSION";
    for (const char* no : values)
        for (const char* val : values) {
            g_val[0] = no; g_val[1] = val;
            char what[96];
            snprintf(what, sizeof(what), "PNR_NO_COMPOSITE_FUSION=\"%s\" PNR_COMPOSITE_FUSION=\"%s\"", no, val);
            if (check_initial(what)) return 1;
        }
    return 0;
}
