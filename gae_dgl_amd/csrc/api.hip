// Library-level entry points: version, error string, device info, tuning knobs.
#include <stdarg.h>
#include <string.h>

#include "common.h"

namespace gae {
static thread_local char g_err[512] = "";
void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
} // namespace gae

namespace {

// Every knob of gae_tuning_set / gae_tuning_get (include/gae_hip.h lists them with their defaults).  A value is
// allowed when it lies in [lo, hi] and, for knobs with a `values` mask, its bit (1 << value) is set there.
struct KnobEntry {
    const char *name;
    gae::Knob *knob;
    int lo, hi;
    unsigned values;    // 0: every value in [lo, hi]
    bool settable;      // false: telemetry, read-only
};

constexpr unsigned V(int a) { return 1u << a; }

const KnobEntry kKnobs[] = {
    {"spmm_variant", &gae::g_spmm_variant, 1, 2, 0, true},
    {"spmm_rpg", &gae::g_spmm_rpg, 0, 2, 0, true},
    {"spmm_tile_vecs", &gae::g_spmm_tile_vecs, -1, 256, 0, true},
    {"spmm_ell", &gae::g_spmm_ell, 0, 2, 0, true},
    {"spmm_ell_rpg", &gae::g_spmm_ell_rpg, 0, 2, 0, true},
    {"spmm_hot", &gae::g_spmm_hot, 0, 1, 0, true},
    {"spmm_desc", &gae::g_spmm_desc, 0, 1, 0, true},
    {"spmm_light", &gae::g_spmm_light, 0, 1, 0, true},
    {"ell_side", &gae::g_ell_side, 0, 15, 0, true},
    {"gemm_rows", &gae::g_gemm_rows, 0, 2, 0, true},
    {"linear_wlds", &gae::g_linear_wlds, 0, 2, 0, true},
    {"atb_bf16", &gae::g_atb_bf16, 0, 2, 0, true},
    {"xw_rows", &gae::g_xw_rows, 0, 1 << 24, 0, true},
    {"xw_parts", &gae::g_xw_parts, 0, 1 << 20, 0, true},
    {"xw_glds", &gae::g_xw_glds, 0, 1, 0, true},
    {"xw_p3", &gae::g_xw_p3, 0, 1, 0, true},
    {"bce_s_bf16", &gae::g_bce_s_bf16, 0, 3, V(0) | V(2) | V(3), true},
    {"bce_pv_bf16", &gae::g_bce_pv_bf16, 0, 1, 0, true},
    {"bce_sym", &gae::g_bce_sym, 0, 2, 0, true},
    {"bce_sym_ri", &gae::g_bce_sym_ri, 0, 4, V(0) | V(2) | V(4), true},
    {"bce_sym_bal", &gae::g_bce_sym_bal, 0, 2, 0, true},
    {"bce_last_kind", &gae::g_bce_last_kind, 0, 3, 0, false},
    {"dense_last_kind", &gae::g_dense_last_kind, 0, 11, 0, false},
    {"topk_splits", &gae::g_topk_splits, 0, 16, 0, true},
    {"rank_splits", &gae::g_rank_splits, 0, 16, 0, true},
};

const KnobEntry *find_knob(const char *name)
{
    for (const KnobEntry &e : kKnobs)
        if (strcmp(e.name, name) == 0) return &e;
    return nullptr;
}

bool allowed(const KnobEntry &e, int64_t v)
{
    return v >= e.lo && v <= e.hi && (e.values == 0 || (e.values >> v) & 1u);
}

} // namespace

extern "C" int gae_tuning_set(const char *name, int64_t value)
{
    GAE_REQUIRE(name != nullptr, GAE_E_NULL, "gae_tuning_set: name is NULL");
    const KnobEntry *e = find_knob(name);
    GAE_REQUIRE(e != nullptr, GAE_E_RANGE, "gae_tuning_set: unknown knob '%s'", name);
    GAE_REQUIRE(e->settable, GAE_E_RANGE, "gae_tuning_set: knob '%s' is read-only", name);
    if (!allowed(*e, value)) {
        char list[128] = "";
        if (e->values) {
            for (int v = e->lo; v <= e->hi; ++v)
                if (allowed(*e, v)) snprintf(list + strlen(list), sizeof(list) - strlen(list), "%s%d", list[0] ? ", " : "", v);
        } else {
            snprintf(list, sizeof(list), "%d .. %d", e->lo, e->hi);
        }
        gae::set_error("gae_tuning_set: %s = %lld is out of range (allowed: %s)", name, (long long)value, list);
        return GAE_E_RANGE;
    }
    *e->knob = int(value);
    return GAE_OK;
}

extern "C" int gae_tuning_get(const char *name, int64_t *value_out)
{
    GAE_REQUIRE(name != nullptr && value_out != nullptr, GAE_E_NULL, "gae_tuning_get: NULL argument");
    const KnobEntry *e = find_knob(name);
    GAE_REQUIRE(e != nullptr, GAE_E_RANGE, "gae_tuning_get: unknown knob '%s'", name);
    *value_out = int(*e->knob);
    return GAE_OK;
}

extern "C" int gae_version(void) { return GAE_VERSION; }

extern "C" const char *gae_last_error(void) { return gae::g_err; }

extern "C" int gae_device_info_get(int device, gae_device_info *out)
{
    GAE_REQUIRE(out != nullptr, GAE_E_NULL, "gae_device_info_get: out is NULL");
    hipDeviceProp_t p;
    GAE_HIP(hipGetDeviceProperties(&p, device));
    memset(out, 0, sizeof(*out));
    out->compute_units = p.multiProcessorCount;
    out->wavefront_size = p.warpSize;
    out->lds_bytes_per_cu = static_cast<int32_t>(p.maxSharedMemoryPerMultiProcessor);
    out->l2_bytes = p.l2CacheSize;
    out->hbm_bytes = static_cast<int64_t>(p.totalGlobalMem);
    out->clock_khz = p.clockRate;
    int gfx = 0;
    const char *a = strstr(p.gcnArchName, "gfx");
    if (a) gfx = atoi(a + 3);
    out->gfx_major_minor = gfx;
    strncpy(out->name, p.name, sizeof(out->name) - 1);
    return GAE_OK;
}
