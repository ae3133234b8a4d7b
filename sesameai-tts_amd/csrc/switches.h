// Every CSM_* / MIMI_* environment switch, host code only.  They exist so the A/Bs can be re-run; none is needed in
// production.  A name under those prefixes that is in neither list selects nothing -- a typo, or a switch that was retired, would silently
// leave the default in force -- so the first csm_create / mimi_create of a process lists such names once on stderr (csm_warn_unknown_switches).
#pragma once
#include <stdlib.h>

// read by the engines, through the three accessors below and nowhere else
#define CSM_ENGINE_SWITCHES(X)                                                                                                              \
    X(CSM_ATTN_MERGE) X(CSM_BB_BLOCK) X(CSM_BB_LAYER) X(CSM_DEC_FIRST) X(CSM_FP8_WIDE) X(CSM_FUSE_DEC_ATTN) X(CSM_G128_MIN_ROWS)             \
    X(CSM_G128_ROWTILES) X(CSM_G256_MIN_ROWS) X(CSM_G64_MAX_BLOCKS) X(CSM_KEEP_FAST_PATHS) X(CSM_MMT_MIN_ROWS) X(CSM_MMT_OPS) X(CSM_PERSIST) \
    X(CSM_PERSIST_FAULT) X(CSM_PERSIST_M) X(CSM_PERSIST_M_MAX) X(CSM_PERSIST_M_TRICKLE) X(CSM_PERSIST_POLL) X(CSM_PERSIST_TRICKLE)           \
    X(CSM_QKV0_TABLE) X(CSM_QUIET) X(CSM_SLAB_K) X(CSM_WIDE) X(CSM_WIDE_MIN) X(CSM_XPACK) X(CSM_XPACK_PROMPT) X(MIMI_GRAPH_MAX_T) X(MIMI_KSPLIT)
// read only by the Python host, the tools or the C examples: known names, nothing here reads them
#define CSM_HOST_SWITCHES(X)                                                                                                                \
    X(CSM_C_HOST_GPUS) X(CSM_HIP_LIB) X(CSM_HIP_TIMELINE) X(CSM_MIMI_PATH) X(CSM_MODEL_PATH) X(CSM_NO_WARMUP) X(CSM_SYNTHETIC)               \
    X(CSM_TOKENIZER_JSON) X(CSM_VOICE_DIR)

#define SW_ID_(name) SW_##name,
#define SW_STR_(name) #name,
enum Switch { CSM_ENGINE_SWITCHES(SW_ID_) SW_ENGINE_COUNT };
static const char* const SWITCH_NAMES[] = {CSM_ENGINE_SWITCHES(SW_STR_) CSM_HOST_SWITCHES(SW_STR_)};      // [0, SW_ENGINE_COUNT) by enum
#undef SW_ID_
#undef SW_STR_

static inline bool sw_on(Switch s) { const char* ev = getenv(SWITCH_NAMES[s]); return !(ev && ev[0] == '0'); }      // default-on flag: NAME=0 clears it
static inline bool sw_set(Switch s) { return getenv(SWITCH_NAMES[s]) != nullptr; }                                   // default-off flag: any value sets it
static inline int sw_int(Switch s, int dflt) { const char* ev = getenv(SWITCH_NAMES[s]); return ev ? atoi(ev) : dflt; }   // integer: atoi of what is set
