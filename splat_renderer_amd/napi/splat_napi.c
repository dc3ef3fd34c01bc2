/*
 * splat_napi.c — thin N-API addon over the C ABI of libsplat_hip.so (include/splat.h).
 *
 * One JS function per ABI entry point, same name without the "splat_" prefix.  Handles (ctx,
 * sorter, binner) are napi_externals; device pointers cross as JS numbers (GPU virtual addresses
 * are < 2^53); host data crosses as TypedArrays/ArrayBuffers.  A negative status becomes a thrown
 * JS Error carrying splat_last_error(), which is the reference's error behaviour (its getters
 * `throw new Error(...)`: /root/reference/src/GPUTileBinner.ts:340-359).
 *
 * Plain C, no node-addon-api, no node-gyp: built by the Makefile next to this file with
 *   gcc -shared -fPIC -I/usr/include/node splat_napi.c -o splat_napi.node -L.. -lsplat_hip
 */
#define NAPI_VERSION 6
#include <node_api.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/splat.h"

#define MAX_ARGS 24

typedef struct {
    napi_env env;
    size_t argc;
    napi_value argv[MAX_ARGS];
    int failed;
} call_t;

static int get_args(napi_env env, napi_callback_info info, call_t *c, size_t want) {
    c->env = env;
    c->argc = MAX_ARGS;
    c->failed = 0;
    if (napi_get_cb_info(env, info, &c->argc, c->argv, NULL, NULL) != napi_ok || c->argc < want) {
        napi_throw_type_error(env, NULL, "wrong number of arguments");
        return 0;
    }
    return 1;
}

static void *arg_external(call_t *c, size_t i) {
    void *p = NULL;
    napi_valuetype t;
    napi_typeof(c->env, c->argv[i], &t);
    if (t == napi_null || t == napi_undefined) return NULL;
    if (napi_get_value_external(c->env, c->argv[i], &p) != napi_ok) {
        c->failed = 1;
        napi_throw_type_error(c->env, NULL, "expected a handle");
    }
    return p;
}

static double arg_number(call_t *c, size_t i) {
    double d = 0;
    if (napi_get_value_double(c->env, c->argv[i], &d) != napi_ok) {
        c->failed = 1;
        napi_throw_type_error(c->env, NULL, "expected a number");
    }
    return d;
}

static void *arg_dptr(call_t *c, size_t i) { /* device pointer as a number; null/undefined -> NULL */
    napi_valuetype t;
    napi_typeof(c->env, c->argv[i], &t);
    if (t == napi_null || t == napi_undefined) return NULL;
    return (void *)(uintptr_t)arg_number(c, i);
}

static void *arg_hostbuf(call_t *c, size_t i, size_t *bytes) { /* TypedArray, DataView or ArrayBuffer */
    bool is = false;
    void *data = NULL;
    size_t len = 0;
    napi_is_typedarray(c->env, c->argv[i], &is);
    if (is) {
        napi_typedarray_type tt;
        napi_value ab;
        size_t off;
        napi_get_typedarray_info(c->env, c->argv[i], &tt, &len, &data, &ab, &off);
        static const size_t esz[] = {1, 1, 1, 2, 2, 4, 4, 4, 8, 8, 8};
        len *= esz[tt];
    } else {
        napi_is_arraybuffer(c->env, c->argv[i], &is);
        if (is) {
            napi_get_arraybuffer_info(c->env, c->argv[i], &data, &len);
        } else {
            c->failed = 1;
            napi_throw_type_error(c->env, NULL, "expected a TypedArray or ArrayBuffer");
        }
    }
    if (bytes) *bytes = len;
    return data;
}

static napi_value mk_number(napi_env env, double v) {
    napi_value r;
    napi_create_double(env, v, &r);
    return r;
}

static napi_value mk_undefined(napi_env env) {
    napi_value r;
    napi_get_undefined(env, &r);
    return r;
}

static napi_value mk_external(napi_env env, void *p) {
    napi_value r;
    napi_create_external(env, p, NULL, NULL, &r);
    return r;
}

/* status -> thrown Error("libsplat_hip <code>: <message>") */
static napi_value check(napi_env env, splat_ctx *ctx, int rc, napi_value ok) {
    if (rc == SPLAT_OK) return ok;
    char msg[600];
    const char *m = splat_last_error(ctx);
    strcpy(msg, "libsplat_hip ");
    char num[16];
    int n = rc, k = 0;
    if (n < 0) { msg[strlen(msg) + 1] = 0; msg[strlen(msg)] = '-'; n = -n; }
    do { num[k++] = (char)('0' + n % 10); n /= 10; } while (n);
    while (k) { size_t l = strlen(msg); msg[l] = num[--k]; msg[l + 1] = 0; }
    strcat(msg, ": ");
    strncat(msg, m ? m : "", sizeof msg - strlen(msg) - 1);
    napi_throw_error(env, NULL, msg);
    return NULL;
}

/* A frame function that returns SPLAT_ERR_CAPACITY / SPLAT_ERR_RETRY is reporting the PREVIOUS (sync-free) frame — it
 * outgrew its pair limit, or its lists failed the order check; room has been made / the ranking switched — and has not
 * rendered this one: call it again (include/splat.h).  The Python facades do the same (host.py Renderer.render). */
#define AGAIN(rc) ((rc) == SPLAT_ERR_CAPACITY || (rc) == SPLAT_ERR_RETRY)

#define FN(name) static napi_value name(napi_env env, napi_callback_info info)
#define ARGS(n) call_t c; if (!get_args(env, info, &c, n)) return NULL
#define BAIL if (c.failed) return NULL

FN(abi_version) { (void)info; return mk_number(env, splat_abi_version()); }

FN(ctx_create) {
    ARGS(1);
    int dev = (int)arg_number(&c, 0); BAIL;
    splat_ctx *ctx = NULL;
    int rc = splat_ctx_create(dev, &ctx);
    return check(env, NULL, rc, rc == SPLAT_OK ? mk_external(env, ctx) : NULL);
}
FN(ctx_destroy) { ARGS(1); splat_ctx_destroy((splat_ctx *)arg_external(&c, 0)); return mk_undefined(env); }
FN(sync) { ARGS(1); splat_ctx *x = arg_external(&c, 0); BAIL; return check(env, x, splat_sync(x), mk_undefined(env)); }
FN(rank_status) { /* (ctx) -> [policy (0 checked | 1 atomic | 2 ballot), atomicsOrdered (1 | 0 | -1), orderFaults]: splat_rank_status */
    ARGS(1); splat_ctx *x = arg_external(&c, 0); BAIL;
    int pol = 0, ordered = 0; uint32_t faults = 0;
    int rc = splat_rank_status(x, &pol, &ordered, &faults);
    if (rc != SPLAT_OK) return check(env, x, rc, NULL);
    napi_value arr;
    if (napi_create_array_with_length(env, 3, &arr) != napi_ok) return NULL;
    napi_set_element(env, arr, 0, mk_number(env, pol));
    napi_set_element(env, arr, 1, mk_number(env, ordered));
    napi_set_element(env, arr, 2, mk_number(env, (double)faults));
    return arr;
}
FN(set_timing) { ARGS(2); splat_ctx *x = arg_external(&c, 0); int e = (int)arg_number(&c, 1); BAIL; return check(env, x, splat_set_timing(x, e), mk_undefined(env)); }
FN(stage_time_ms) {
    ARGS(2); splat_ctx *x = arg_external(&c, 0); int st = (int)arg_number(&c, 1); BAIL;
    float ms = 0; int rc = splat_stage_time_ms(x, st, &ms);
    return check(env, x, rc, mk_number(env, ms));
}
FN(buf_alloc) {
    ARGS(2); splat_ctx *x = arg_external(&c, 0); size_t b = (size_t)arg_number(&c, 1); BAIL;
    void *p = NULL; int rc = splat_buf_alloc(x, b, &p);
    return check(env, x, rc, mk_number(env, (double)(uintptr_t)p));
}
FN(buf_free) { ARGS(2); splat_ctx *x = arg_external(&c, 0); void *p = arg_dptr(&c, 1); BAIL; return check(env, x, splat_buf_free(x, p), mk_undefined(env)); }
FN(buf_zero) { ARGS(3); splat_ctx *x = arg_external(&c, 0); void *p = arg_dptr(&c, 1); size_t b = (size_t)arg_number(&c, 2); BAIL; return check(env, x, splat_buf_zero(x, p, b), mk_undefined(env)); }
FN(buf_upload) { /* (ctx, dptr, hostTypedArray) */
    ARGS(3); splat_ctx *x = arg_external(&c, 0); void *p = arg_dptr(&c, 1); size_t n = 0; void *h = arg_hostbuf(&c, 2, &n); BAIL;
    return check(env, x, splat_buf_upload(x, p, h, n), mk_undefined(env));
}
FN(buf_download) { /* (ctx, hostTypedArray, dptr) fills the whole array */
    ARGS(3); splat_ctx *x = arg_external(&c, 0); size_t n = 0; void *h = arg_hostbuf(&c, 1, &n); void *p = arg_dptr(&c, 2); BAIL;
    return check(env, x, splat_buf_download(x, h, p, n), mk_undefined(env));
}
FN(update_props) {
    ARGS(5); splat_ctx *x = arg_external(&c, 0); void *pos = arg_dptr(&c, 1), *cur = arg_dptr(&c, 2);
    uint32_t n = (uint32_t)arg_number(&c, 3); void *props = arg_dptr(&c, 4); BAIL;
    return check(env, x, splat_update_props(x, pos, cur, n, props), mk_undefined(env));
}
FN(update_props_planes) { /* (ctx, positions, curvature, n, posRadius, colorOpacity) */
    ARGS(6); splat_ctx *x = arg_external(&c, 0); void *pos = arg_dptr(&c, 1), *cur = arg_dptr(&c, 2);
    uint32_t n = (uint32_t)arg_number(&c, 3); void *pr = arg_dptr(&c, 4), *co = arg_dptr(&c, 5); BAIL;
    return check(env, x, splat_update_props_planes(x, pos, cur, n, pr, co), mk_undefined(env));
}
FN(props_to_planes) { /* (ctx, props, n, posRadius, colorOpacity) */
    ARGS(5); splat_ctx *x = arg_external(&c, 0); void *props = arg_dptr(&c, 1); uint32_t n = (uint32_t)arg_number(&c, 2);
    void *pr = arg_dptr(&c, 3), *co = arg_dptr(&c, 4); BAIL;
    return check(env, x, splat_props_to_planes(x, props, n, pr, co), mk_undefined(env));
}
FN(lit_colors) { /* (ctx, colorOpacity, cStride, normals, nStride, n, lit) */
    ARGS(7); splat_ctx *x = arg_external(&c, 0); void *col = arg_dptr(&c, 1); uint32_t cs = (uint32_t)arg_number(&c, 2);
    void *nrm = arg_dptr(&c, 3); uint32_t ns = (uint32_t)arg_number(&c, 4), n = (uint32_t)arg_number(&c, 5); void *lit = arg_dptr(&c, 6); BAIL;
    return check(env, x, splat_lit_colors(x, col, cs, nrm, ns, n, lit), mk_undefined(env));
}
FN(project) { /* (ctx, Float32Array(22), posRadius, strideVec4, n, projected, keys|null, payload|null, nPadded) */
    ARGS(9); splat_ctx *x = arg_external(&c, 0); size_t ub = 0; float *u = arg_hostbuf(&c, 1, &ub);
    void *pr = arg_dptr(&c, 2); uint32_t st = (uint32_t)arg_number(&c, 3), n = (uint32_t)arg_number(&c, 4);
    void *proj = arg_dptr(&c, 5), *keys = arg_dptr(&c, 6), *pay = arg_dptr(&c, 7); uint32_t np = (uint32_t)arg_number(&c, 8); BAIL;
    if (ub < 22 * sizeof(float)) { napi_throw_range_error(env, NULL, "uniform block needs 22 floats"); return NULL; }
    return check(env, x, splat_project(x, u, pr, st, n, proj, keys, pay, np), mk_undefined(env));
}
FN(project_disc) { /* (ctx, Float32Array(22), posRadius, strideVec4, normals, normalStrideVec4, n, projected, discs, keys|null, payload|null, nPadded) */
    ARGS(12); splat_ctx *x = arg_external(&c, 0); size_t ub = 0; float *u = arg_hostbuf(&c, 1, &ub);
    void *pr = arg_dptr(&c, 2); uint32_t st = (uint32_t)arg_number(&c, 3); void *nrm = arg_dptr(&c, 4);
    uint32_t ns = (uint32_t)arg_number(&c, 5), n = (uint32_t)arg_number(&c, 6);
    void *proj = arg_dptr(&c, 7), *discs = arg_dptr(&c, 8), *keys = arg_dptr(&c, 9), *pay = arg_dptr(&c, 10); uint32_t np = (uint32_t)arg_number(&c, 11); BAIL;
    if (ub < 22 * sizeof(float)) { napi_throw_range_error(env, NULL, "uniform block needs 22 floats"); return NULL; }
    return check(env, x, splat_project_disc(x, u, pr, st, nrm, ns, n, proj, discs, keys, pay, np), mk_undefined(env));
}
FN(extract_keys) {
    ARGS(6); splat_ctx *x = arg_external(&c, 0); void *proj = arg_dptr(&c, 1); uint32_t n = (uint32_t)arg_number(&c, 2), np = (uint32_t)arg_number(&c, 3);
    void *k = arg_dptr(&c, 4), *p = arg_dptr(&c, 5); BAIL;
    return check(env, x, splat_extract_keys(x, proj, n, np, k, p), mk_undefined(env));
}
FN(sort_create) {
    ARGS(2); splat_ctx *x = arg_external(&c, 0); uint32_t cap = (uint32_t)arg_number(&c, 1); BAIL;
    splat_sorter *s = NULL; int rc = splat_sort_create(x, cap, &s);
    return check(env, x, rc, rc == SPLAT_OK ? mk_external(env, s) : NULL);
}
FN(sort_destroy) { ARGS(1); splat_sort_destroy(arg_external(&c, 0)); return mk_undefined(env); }
FN(sort_capacity) { ARGS(1); return mk_number(env, splat_sort_capacity(arg_external(&c, 0))); }
FN(sort_keys) { ARGS(1); return mk_number(env, (double)(uintptr_t)splat_sort_keys(arg_external(&c, 0))); }
FN(sort_payload) { ARGS(1); return mk_number(env, (double)(uintptr_t)splat_sort_payload(arg_external(&c, 0))); }
FN(sort_sorted_payload) { ARGS(1); return mk_number(env, (double)(uintptr_t)splat_sort_sorted_payload(arg_external(&c, 0))); }
FN(sort_sorted_keys) { ARGS(1); return mk_number(env, (double)(uintptr_t)splat_sort_sorted_keys(arg_external(&c, 0))); }
FN(sort_run) { /* (ctx, sorter, n, bitBegin, bitEnd) */
    ARGS(5); splat_ctx *x = arg_external(&c, 0); splat_sorter *s = arg_external(&c, 1);
    uint32_t n = (uint32_t)arg_number(&c, 2), b0 = (uint32_t)arg_number(&c, 3), b1 = (uint32_t)arg_number(&c, 4); BAIL;
    return check(env, x, splat_sort_run(s, n, b0, b1), mk_undefined(env));
}
FN(sort_set_mode) { ARGS(3); splat_ctx *x = arg_external(&c, 0); splat_sorter *s = arg_external(&c, 1); int m = (int)arg_number(&c, 2); BAIL; return check(env, x, splat_sort_set_mode(s, m), mk_undefined(env)); }
FN(bin_set_frame_order) { ARGS(3); splat_ctx *x = arg_external(&c, 0); splat_binner *b = arg_external(&c, 1); int o = (int)arg_number(&c, 2); BAIL; return check(env, x, splat_bin_set_frame_order(b, o), mk_undefined(env)); }
FN(scan_u32) {
    ARGS(5); splat_ctx *x = arg_external(&c, 0); void *in = arg_dptr(&c, 1), *out = arg_dptr(&c, 2); uint32_t n = (uint32_t)arg_number(&c, 3);
    void *tot = arg_dptr(&c, 4); BAIL;
    return check(env, x, splat_scan_u32(x, in, out, n, tot), mk_undefined(env));
}
FN(bin_create) {
    ARGS(2); splat_ctx *x = arg_external(&c, 0); uint32_t t = (uint32_t)arg_number(&c, 1); BAIL;
    splat_binner *b = NULL; int rc = splat_bin_create(x, t, &b);
    return check(env, x, rc, rc == SPLAT_OK ? mk_external(env, b) : NULL);
}
FN(bin_destroy) { ARGS(1); splat_bin_destroy(arg_external(&c, 0)); return mk_undefined(env); }
FN(bin_run) { /* (ctx, binner, projected, nSplats, sorted, nSorted, W, H, row0, row1) */
    ARGS(10); splat_ctx *x = arg_external(&c, 0); splat_binner *b = arg_external(&c, 1); void *proj = arg_dptr(&c, 2);
    uint32_t ns = (uint32_t)arg_number(&c, 3); void *sorted = arg_dptr(&c, 4); uint32_t nso = (uint32_t)arg_number(&c, 5);
    uint32_t w = (uint32_t)arg_number(&c, 6), h = (uint32_t)arg_number(&c, 7), r0 = (uint32_t)arg_number(&c, 8), r1 = (uint32_t)arg_number(&c, 9); BAIL;
    return check(env, x, splat_bin_run(b, proj, ns, sorted, nso, w, h, r0, r1), mk_undefined(env));
}
#define BIN_GETTER(jsname, cfn)                                                                        \
    FN(jsname) {                                                                                       \
        ARGS(2); splat_ctx *x = arg_external(&c, 0); splat_binner *b = arg_external(&c, 1); BAIL;      \
        void *p = NULL; int rc = cfn(b, &p);                                                           \
        return check(env, x, rc, mk_number(env, (double)(uintptr_t)p));                                \
    }
BIN_GETTER(bin_counts, splat_bin_counts)
BIN_GETTER(bin_offsets, splat_bin_offsets)
BIN_GETTER(bin_indices, splat_bin_indices)
FN(bin_total) {
    ARGS(2); splat_ctx *x = arg_external(&c, 0); splat_binner *b = arg_external(&c, 1); BAIL;
    uint64_t t = 0; int rc = splat_bin_total(b, &t);
    return check(env, x, rc, mk_number(env, (double)t));
}
FN(validate_tile_order) { /* (ctx, projected, offsets, numTiles, indices, totalPairs) -> violations */
    ARGS(6); splat_ctx *x = arg_external(&c, 0); void *proj = arg_dptr(&c, 1), *off = arg_dptr(&c, 2); uint32_t nt = (uint32_t)arg_number(&c, 3);
    void *idx = arg_dptr(&c, 4); uint64_t total = (uint64_t)arg_number(&c, 5); BAIL;
    uint64_t v = 0; int rc = splat_validate_tile_order(x, proj, off, nt, idx, total, &v);
    return check(env, x, rc, mk_number(env, (double)v));
}
static void fill_cfg(call_t *c, size_t i, splat_composite_cfg *cfg) { /* [mode, earlyOut, tile, row0, row1, recordFormat?, prelit?, footprint?] */
    memset(cfg, 0, sizeof *cfg);
    uint32_t v[8] = {0, 1, 16, 0, 0xffffffffu, 0, 0, 0};
    bool is = false;
    napi_is_array(c->env, c->argv[i], &is);
    if (is)
        for (uint32_t k = 0; k < 8; ++k) {
            napi_value e;
            double d;
            if (napi_get_element(c->env, c->argv[i], k, &e) == napi_ok && napi_get_value_double(c->env, e, &d) == napi_ok) v[k] = (uint32_t)d;
        }
    cfg->mode = v[0]; cfg->early_out = v[1]; cfg->tile_size = v[2]; cfg->tile_row0 = v[3]; cfg->tile_row1 = v[4];
    cfg->record_format = v[5]; cfg->prelit = v[6]; cfg->footprint = v[7];
}
FN(composite) { /* (ctx, cfg[5], color, cStride, normals, nStride, projected, indices, counts, offsets, W, H, out8|null, outF|null) */
    ARGS(14); splat_ctx *x = arg_external(&c, 0); splat_composite_cfg cfg; fill_cfg(&c, 1, &cfg);
    void *col = arg_dptr(&c, 2); uint32_t cs = (uint32_t)arg_number(&c, 3); void *nrm = arg_dptr(&c, 4); uint32_t ns = (uint32_t)arg_number(&c, 5);
    void *proj = arg_dptr(&c, 6), *idx = arg_dptr(&c, 7), *cnt = arg_dptr(&c, 8), *off = arg_dptr(&c, 9);
    uint32_t w = (uint32_t)arg_number(&c, 10), h = (uint32_t)arg_number(&c, 11); void *o8 = arg_dptr(&c, 12), *of = arg_dptr(&c, 13); BAIL;
    return check(env, x, splat_composite(x, &cfg, col, cs, nrm, ns, proj, idx, cnt, off, w, h, o8, of, NULL), mk_undefined(env));
}
/* splat_aov from [depth|null, alpha|null, ids|null] (device pointers); undefined / null: no auxiliary outputs */
static splat_aov *fill_aov(call_t *c, size_t i, splat_aov *aov) {
    memset(aov, 0, sizeof *aov);
    bool is = false;
    napi_is_array(c->env, c->argv[i], &is);
    if (!is) return NULL;
    void **slot[3] = {&aov->depth_f32, &aov->alpha_f32, &aov->id_u32};
    for (uint32_t k = 0; k < 3; ++k) {
        napi_value e;
        napi_valuetype t = napi_undefined;
        if (napi_get_element(c->env, c->argv[i], k, &e) != napi_ok) continue;
        napi_typeof(c->env, e, &t);
        double d = 0; /* a device pointer as a number, as arg_dptr takes it */
        if (t == napi_number && napi_get_value_double(c->env, e, &d) == napi_ok) *slot[k] = (void *)(uintptr_t)d;
    }
    return aov;
}
FN(composite_aov) { /* (ctx, cfg[5], color, cStride, normals, nStride, projected, indices, counts, offsets, W, H, out8|null, outF|null, [depth, alpha, ids]) */
    ARGS(15); splat_ctx *x = arg_external(&c, 0); splat_composite_cfg cfg; fill_cfg(&c, 1, &cfg);
    void *col = arg_dptr(&c, 2); uint32_t cs = (uint32_t)arg_number(&c, 3); void *nrm = arg_dptr(&c, 4); uint32_t ns = (uint32_t)arg_number(&c, 5);
    void *proj = arg_dptr(&c, 6), *idx = arg_dptr(&c, 7), *cnt = arg_dptr(&c, 8), *off = arg_dptr(&c, 9);
    uint32_t w = (uint32_t)arg_number(&c, 10), h = (uint32_t)arg_number(&c, 11); void *o8 = arg_dptr(&c, 12), *of = arg_dptr(&c, 13); BAIL;
    splat_aov a; const splat_aov *ap = fill_aov(&c, 14, &a);
    return check(env, x, splat_composite_aov(x, &cfg, col, cs, nrm, ns, proj, idx, cnt, off, w, h, o8, of, NULL, ap), mk_undefined(env));
}
FN(composite_aov_depth) { /* composite_aov's arguments, then depth (device pointer), depthStrideFloats */
    ARGS(17); splat_ctx *x = arg_external(&c, 0); splat_composite_cfg cfg; fill_cfg(&c, 1, &cfg);
    void *col = arg_dptr(&c, 2); uint32_t cs = (uint32_t)arg_number(&c, 3); void *nrm = arg_dptr(&c, 4); uint32_t ns = (uint32_t)arg_number(&c, 5);
    void *proj = arg_dptr(&c, 6), *idx = arg_dptr(&c, 7), *cnt = arg_dptr(&c, 8), *off = arg_dptr(&c, 9);
    uint32_t w = (uint32_t)arg_number(&c, 10), h = (uint32_t)arg_number(&c, 11); void *o8 = arg_dptr(&c, 12), *of = arg_dptr(&c, 13);
    void *z = arg_dptr(&c, 15); uint32_t zs = (uint32_t)arg_number(&c, 16); BAIL;
    splat_aov a; const splat_aov *ap = fill_aov(&c, 14, &a);
    return check(env, x, splat_composite_aov_depth(x, &cfg, col, cs, nrm, ns, proj, idx, cnt, off, w, h, o8, of, NULL, ap, z, zs), mk_undefined(env));
}
FN(render_frame_aov) { /* render_frame's arguments, then [depth, alpha, ids] */
    ARGS(14); splat_ctx *x = arg_external(&c, 0); splat_sorter *s = arg_external(&c, 1); splat_binner *b = arg_external(&c, 2);
    splat_composite_cfg cfg; fill_cfg(&c, 3, &cfg); size_t ub = 0; float *u = arg_hostbuf(&c, 4, &ub);
    void *props = arg_dptr(&c, 5), *nrm = arg_dptr(&c, 6); uint32_t n = (uint32_t)arg_number(&c, 7), w = (uint32_t)arg_number(&c, 8), h = (uint32_t)arg_number(&c, 9);
    void *proj = arg_dptr(&c, 10), *o8 = arg_dptr(&c, 11), *of = arg_dptr(&c, 12); BAIL;
    splat_aov a; const splat_aov *ap = fill_aov(&c, 13, &a);
    if (ub < 22 * sizeof(float)) { napi_throw_range_error(env, NULL, "uniform block needs 22 floats"); return NULL; }
    int rc = splat_render_frame_aov(x, s, b, &cfg, u, props, nrm, n, w, h, proj, o8, of, ap);
    if (AGAIN(rc)) rc = splat_render_frame_aov(x, s, b, &cfg, u, props, nrm, n, w, h, proj, o8, of, ap);
    return check(env, x, rc, mk_undefined(env));
}
FN(render_frame_planes_aov) { /* render_frame_planes' arguments, then [depth, alpha, ids] */
    ARGS(15); splat_ctx *x = arg_external(&c, 0); splat_sorter *s = arg_external(&c, 1); splat_binner *b = arg_external(&c, 2);
    splat_composite_cfg cfg; fill_cfg(&c, 3, &cfg); size_t ub = 0; float *u = arg_hostbuf(&c, 4, &ub);
    void *pr = arg_dptr(&c, 5), *co = arg_dptr(&c, 6), *nrm = arg_dptr(&c, 7);
    uint32_t n = (uint32_t)arg_number(&c, 8), w = (uint32_t)arg_number(&c, 9), h = (uint32_t)arg_number(&c, 10);
    void *proj = arg_dptr(&c, 11), *o8 = arg_dptr(&c, 12), *of = arg_dptr(&c, 13); BAIL;
    splat_aov a; const splat_aov *ap = fill_aov(&c, 14, &a);
    if (ub < 22 * sizeof(float)) { napi_throw_range_error(env, NULL, "uniform block needs 22 floats"); return NULL; }
    int rc = splat_render_frame_planes_aov(x, s, b, &cfg, u, pr, co, nrm, n, w, h, proj, o8, of, ap);
    if (AGAIN(rc)) rc = splat_render_frame_planes_aov(x, s, b, &cfg, u, pr, co, nrm, n, w, h, proj, o8, of, ap);
    return check(env, x, rc, mk_undefined(env));
}
FN(project_ellipsoid) { /* (ctx, Float32Array(22), positions, posStride, scales, scaleStride, rotations, rotStride, n, projected, records, keys|null, payload|null, nPadded) */
    ARGS(14); splat_ctx *x = arg_external(&c, 0); size_t ub = 0; float *u = arg_hostbuf(&c, 1, &ub);
    void *pos = arg_dptr(&c, 2); uint32_t ps = (uint32_t)arg_number(&c, 3); void *scl = arg_dptr(&c, 4); uint32_t ss = (uint32_t)arg_number(&c, 5);
    void *rot = arg_dptr(&c, 6); uint32_t rs = (uint32_t)arg_number(&c, 7), n = (uint32_t)arg_number(&c, 8);
    void *proj = arg_dptr(&c, 9), *rec = arg_dptr(&c, 10), *keys = arg_dptr(&c, 11), *pay = arg_dptr(&c, 12); uint32_t np = (uint32_t)arg_number(&c, 13); BAIL;
    if (ub < 22 * sizeof(float)) { napi_throw_range_error(env, NULL, "uniform block needs 22 floats"); return NULL; }
    return check(env, x, splat_project_ellipsoid(x, u, pos, ps, scl, ss, rot, rs, n, proj, rec, keys, pay, np), mk_undefined(env));
}
FN(project_ellipsoid_aa) { /* project_ellipsoid's arguments, then rho|null, colorOpacity|null, colorStride, colorOpacityOut|null */
    ARGS(18); splat_ctx *x = arg_external(&c, 0); size_t ub = 0; float *u = arg_hostbuf(&c, 1, &ub);
    void *pos = arg_dptr(&c, 2); uint32_t ps = (uint32_t)arg_number(&c, 3); void *scl = arg_dptr(&c, 4); uint32_t ss = (uint32_t)arg_number(&c, 5);
    void *rot = arg_dptr(&c, 6); uint32_t rs = (uint32_t)arg_number(&c, 7), n = (uint32_t)arg_number(&c, 8);
    void *proj = arg_dptr(&c, 9), *rec = arg_dptr(&c, 10), *keys = arg_dptr(&c, 11), *pay = arg_dptr(&c, 12); uint32_t np = (uint32_t)arg_number(&c, 13);
    void *rho = arg_dptr(&c, 14), *co = arg_dptr(&c, 15); uint32_t cs = (uint32_t)arg_number(&c, 16); void *coo = arg_dptr(&c, 17); BAIL;
    if (ub < 22 * sizeof(float)) { napi_throw_range_error(env, NULL, "uniform block needs 22 floats"); return NULL; }
    return check(env, x, splat_project_ellipsoid_aa(x, u, pos, ps, scl, ss, rot, rs, n, proj, rec, keys, pay, np, rho, co, cs, coo), mk_undefined(env));
}
FN(project_surfel) { /* project_ellipsoid's arguments, then clipW|null */
    ARGS(15); splat_ctx *x = arg_external(&c, 0); size_t ub = 0; float *u = arg_hostbuf(&c, 1, &ub);
    void *pos = arg_dptr(&c, 2); uint32_t ps = (uint32_t)arg_number(&c, 3); void *scl = arg_dptr(&c, 4); uint32_t ss = (uint32_t)arg_number(&c, 5);
    void *rot = arg_dptr(&c, 6); uint32_t rs = (uint32_t)arg_number(&c, 7), n = (uint32_t)arg_number(&c, 8);
    void *proj = arg_dptr(&c, 9), *rec = arg_dptr(&c, 10), *keys = arg_dptr(&c, 11), *pay = arg_dptr(&c, 12); uint32_t np = (uint32_t)arg_number(&c, 13);
    void *cw = arg_dptr(&c, 14); BAIL;
    if (ub < 22 * sizeof(float)) { napi_throw_range_error(env, NULL, "uniform block needs 22 floats"); return NULL; }
    return check(env, x, splat_project_surfel(x, u, pos, ps, scl, ss, rot, rs, n, proj, rec, keys, pay, np, cw), mk_undefined(env));
}
FN(composite_surfel_depth) { /* (ctx, cfg[8], colorOpacity, cStride, records, indices, counts, offsets, W, H, depth, depthStrideFloats, n, outDepth, outAlpha|null) */
    ARGS(15); splat_ctx *x = arg_external(&c, 0); splat_composite_cfg cfg; fill_cfg(&c, 1, &cfg);
    void *col = arg_dptr(&c, 2); uint32_t cs = (uint32_t)arg_number(&c, 3); void *rec = arg_dptr(&c, 4);
    void *idx = arg_dptr(&c, 5), *cnt = arg_dptr(&c, 6), *off = arg_dptr(&c, 7);
    uint32_t w = (uint32_t)arg_number(&c, 8), h = (uint32_t)arg_number(&c, 9); void *z = arg_dptr(&c, 10);
    uint32_t zs = (uint32_t)arg_number(&c, 11), n = (uint32_t)arg_number(&c, 12); void *od = arg_dptr(&c, 13), *oa = arg_dptr(&c, 14); BAIL;
    return check(env, x, splat_composite_surfel_depth(x, &cfg, col, cs, rec, idx, cnt, off, w, h, z, zs, n, od, oa), mk_undefined(env));
}
FN(composite_surfel_distortion) { /* composite_surfel_depth's arguments (outDepth|null, outAlpha|null), then near, far, outDistortion */
    ARGS(18); splat_ctx *x = arg_external(&c, 0); splat_composite_cfg cfg; fill_cfg(&c, 1, &cfg);
    void *col = arg_dptr(&c, 2); uint32_t cs = (uint32_t)arg_number(&c, 3); void *rec = arg_dptr(&c, 4);
    void *idx = arg_dptr(&c, 5), *cnt = arg_dptr(&c, 6), *off = arg_dptr(&c, 7);
    uint32_t w = (uint32_t)arg_number(&c, 8), h = (uint32_t)arg_number(&c, 9); void *z = arg_dptr(&c, 10);
    uint32_t zs = (uint32_t)arg_number(&c, 11), n = (uint32_t)arg_number(&c, 12); void *od = arg_dptr(&c, 13), *oa = arg_dptr(&c, 14);
    float near_ = (float)arg_number(&c, 15), far_ = (float)arg_number(&c, 16); void *odist = arg_dptr(&c, 17); BAIL;
    return check(env, x, splat_composite_surfel_distortion(x, &cfg, col, cs, rec, idx, cnt, off, w, h, z, zs, n, od, oa, near_, far_, odist),
                 mk_undefined(env));
}
FN(composite_backward_distortion) { /* composite_backward_depth's arguments (gradDepthImage|null), then near, far, gradDistortionImage */
    ARGS(21); splat_ctx *x = arg_external(&c, 0); splat_composite_cfg cfg; fill_cfg(&c, 1, &cfg);
    void *col = arg_dptr(&c, 2); uint32_t cs = (uint32_t)arg_number(&c, 3); void *rec = arg_dptr(&c, 4);
    void *idx = arg_dptr(&c, 5), *cnt = arg_dptr(&c, 6), *off = arg_dptr(&c, 7);
    uint32_t w = (uint32_t)arg_number(&c, 8), h = (uint32_t)arg_number(&c, 9); void *gimg = arg_dptr(&c, 10);
    uint32_t n = (uint32_t)arg_number(&c, 11); void *grec = arg_dptr(&c, 12), *gcol = arg_dptr(&c, 13);
    void *z = arg_dptr(&c, 14); uint32_t zs = (uint32_t)arg_number(&c, 15); void *gdimg = arg_dptr(&c, 16), *gz = arg_dptr(&c, 17);
    float near_ = (float)arg_number(&c, 18), far_ = (float)arg_number(&c, 19); void *gdist = arg_dptr(&c, 20); BAIL;
    return check(env, x, splat_composite_backward_distortion(x, &cfg, col, cs, rec, idx, cnt, off, w, h, gimg, n, grec, gcol, z, zs, gdimg, gz,
                                                             near_, far_, gdist), mk_undefined(env));
}
FN(project_surfel_backward) { /* (ctx, Float32Array(22), positions, posStride, scales, scaleStride, rotations, rotStride, n, gradRecords, gradClipW|null, gradPositions, gradScales, gradRotations) */
    ARGS(14); splat_ctx *x = arg_external(&c, 0); size_t ub = 0; float *u = arg_hostbuf(&c, 1, &ub);
    void *pos = arg_dptr(&c, 2); uint32_t ps = (uint32_t)arg_number(&c, 3); void *scl = arg_dptr(&c, 4); uint32_t ss = (uint32_t)arg_number(&c, 5);
    void *rot = arg_dptr(&c, 6); uint32_t rs = (uint32_t)arg_number(&c, 7), n = (uint32_t)arg_number(&c, 8);
    void *grec = arg_dptr(&c, 9), *gcw = arg_dptr(&c, 10), *gp = arg_dptr(&c, 11), *gs = arg_dptr(&c, 12), *gr = arg_dptr(&c, 13); BAIL;
    if (ub < 22 * sizeof(float)) { napi_throw_range_error(env, NULL, "uniform block needs 22 floats"); return NULL; }
    return check(env, x, splat_project_surfel_backward(x, u, pos, ps, scl, ss, rot, rs, n, grec, gcw, gp, gs, gr), mk_undefined(env));
}
FN(sampling_rate_max) { /* (ctx, Float32Array(22), focalPx, near, margin, positions, posStride, n, rateInOut) */
    ARGS(9); splat_ctx *x = arg_external(&c, 0); size_t ub = 0; float *u = arg_hostbuf(&c, 1, &ub);
    float focal = (float)arg_number(&c, 2), near_ = (float)arg_number(&c, 3), margin = (float)arg_number(&c, 4);
    void *pos = arg_dptr(&c, 5); uint32_t ps = (uint32_t)arg_number(&c, 6), n = (uint32_t)arg_number(&c, 7); void *rate = arg_dptr(&c, 8); BAIL;
    if (ub < 22 * sizeof(float)) { napi_throw_range_error(env, NULL, "uniform block needs 22 floats"); return NULL; }
    return check(env, x, splat_sampling_rate_max(x, u, focal, near_, margin, pos, ps, n, rate), mk_undefined(env));
}
FN(sh_colors) { /* (ctx, Float32Array(3) eye, positions, posStride, sh, shStrideFloats, degree, opacity, n, colorOpacityOut) */
    ARGS(10); splat_ctx *x = arg_external(&c, 0); size_t eb = 0; float *eye = arg_hostbuf(&c, 1, &eb);
    void *pos = arg_dptr(&c, 2); uint32_t ps = (uint32_t)arg_number(&c, 3); void *sh = arg_dptr(&c, 4);
    uint32_t shs = (uint32_t)arg_number(&c, 5), deg = (uint32_t)arg_number(&c, 6); void *op = arg_dptr(&c, 7);
    uint32_t n = (uint32_t)arg_number(&c, 8); void *out = arg_dptr(&c, 9); BAIL;
    if (eb < 3 * sizeof(float)) { napi_throw_range_error(env, NULL, "eye needs 3 floats"); return NULL; }
    return check(env, x, splat_sh_colors(x, eye, pos, ps, sh, shs, deg, op, n, out), mk_undefined(env));
}
FN(composite_backward) { /* (ctx, cfg[8], colorOpacity, cStride, records, indices, counts, offsets, W, H, gradRgba32f, n, gradRecords, gradColorOpacity) */
    ARGS(14); splat_ctx *x = arg_external(&c, 0); splat_composite_cfg cfg; fill_cfg(&c, 1, &cfg);
    void *col = arg_dptr(&c, 2); uint32_t cs = (uint32_t)arg_number(&c, 3); void *rec = arg_dptr(&c, 4);
    void *idx = arg_dptr(&c, 5), *cnt = arg_dptr(&c, 6), *off = arg_dptr(&c, 7);
    uint32_t w = (uint32_t)arg_number(&c, 8), h = (uint32_t)arg_number(&c, 9); void *gimg = arg_dptr(&c, 10);
    uint32_t n = (uint32_t)arg_number(&c, 11); void *grec = arg_dptr(&c, 12), *gcol = arg_dptr(&c, 13); BAIL;
    return check(env, x, splat_composite_backward(x, &cfg, col, cs, rec, idx, cnt, off, w, h, gimg, n, grec, gcol), mk_undefined(env));
}
FN(composite_backward_depth) { /* composite_backward's arguments, then depth, depthStrideFloats, gradDepthImage, gradDepth */
    ARGS(18); splat_ctx *x = arg_external(&c, 0); splat_composite_cfg cfg; fill_cfg(&c, 1, &cfg);
    void *col = arg_dptr(&c, 2); uint32_t cs = (uint32_t)arg_number(&c, 3); void *rec = arg_dptr(&c, 4);
    void *idx = arg_dptr(&c, 5), *cnt = arg_dptr(&c, 6), *off = arg_dptr(&c, 7);
    uint32_t w = (uint32_t)arg_number(&c, 8), h = (uint32_t)arg_number(&c, 9); void *gimg = arg_dptr(&c, 10);
    uint32_t n = (uint32_t)arg_number(&c, 11); void *grec = arg_dptr(&c, 12), *gcol = arg_dptr(&c, 13);
    void *z = arg_dptr(&c, 14); uint32_t zs = (uint32_t)arg_number(&c, 15); void *gdimg = arg_dptr(&c, 16), *gz = arg_dptr(&c, 17); BAIL;
    return check(env, x, splat_composite_backward_depth(x, &cfg, col, cs, rec, idx, cnt, off, w, h, gimg, n, grec, gcol, z, zs, gdimg, gz),
                 mk_undefined(env));
}
FN(composite_backward_det_workspace_bytes) { /* (totalPairs, numTiles, n, withDepth) -> bytes */
    ARGS(4); uint64_t pairs = (uint64_t)arg_number(&c, 0); uint32_t tiles = (uint32_t)arg_number(&c, 1), n = (uint32_t)arg_number(&c, 2);
    int depth = (int)arg_number(&c, 3); BAIL;
    return mk_number(env, (double)splat_composite_backward_det_workspace_bytes(pairs, tiles, n, depth));
}
FN(composite_backward_det) { /* (ctx, cfg[8], colorOpacity, cStride, records, projected, indices, counts, offsets, totalPairs, W, H, gradRgba32f, n, gradRecords, gradColorOpacity, depth|null, depthStrideFloats, gradDepthImage|null, gradDepth|null, workspace, workspaceBytes) */
    ARGS(22); splat_ctx *x = arg_external(&c, 0); splat_composite_cfg cfg; fill_cfg(&c, 1, &cfg);
    void *col = arg_dptr(&c, 2); uint32_t cs = (uint32_t)arg_number(&c, 3); void *rec = arg_dptr(&c, 4), *proj = arg_dptr(&c, 5);
    void *idx = arg_dptr(&c, 6), *cnt = arg_dptr(&c, 7), *off = arg_dptr(&c, 8); uint64_t pairs = (uint64_t)arg_number(&c, 9);
    uint32_t w = (uint32_t)arg_number(&c, 10), h = (uint32_t)arg_number(&c, 11); void *gimg = arg_dptr(&c, 12);
    uint32_t n = (uint32_t)arg_number(&c, 13); void *grec = arg_dptr(&c, 14), *gcol = arg_dptr(&c, 15);
    void *z = arg_dptr(&c, 16); uint32_t zs = (uint32_t)arg_number(&c, 17); void *gdimg = arg_dptr(&c, 18), *gz = arg_dptr(&c, 19);
    void *ws = arg_dptr(&c, 20); uint64_t wb = (uint64_t)arg_number(&c, 21); BAIL;
    return check(env, x, splat_composite_backward_det(x, &cfg, col, cs, rec, proj, idx, cnt, off, pairs, w, h, gimg, n, grec, gcol, z, zs, gdimg, gz,
                                                      ws, wb), mk_undefined(env));
}
FN(composite_backward_abs) { /* composite_backward_depth's arguments (depth|null, depthStrideFloats, gradDepthImage|null, gradDepth|null), then gradCenterAbs */
    ARGS(19); splat_ctx *x = arg_external(&c, 0); splat_composite_cfg cfg; fill_cfg(&c, 1, &cfg);
    void *col = arg_dptr(&c, 2); uint32_t cs = (uint32_t)arg_number(&c, 3); void *rec = arg_dptr(&c, 4);
    void *idx = arg_dptr(&c, 5), *cnt = arg_dptr(&c, 6), *off = arg_dptr(&c, 7);
    uint32_t w = (uint32_t)arg_number(&c, 8), h = (uint32_t)arg_number(&c, 9); void *gimg = arg_dptr(&c, 10);
    uint32_t n = (uint32_t)arg_number(&c, 11); void *grec = arg_dptr(&c, 12), *gcol = arg_dptr(&c, 13);
    void *z = arg_dptr(&c, 14); uint32_t zs = (uint32_t)arg_number(&c, 15); void *gdimg = arg_dptr(&c, 16), *gz = arg_dptr(&c, 17);
    void *gabs = arg_dptr(&c, 18); BAIL;
    return check(env, x, splat_composite_backward_abs(x, &cfg, col, cs, rec, idx, cnt, off, w, h, gimg, n, grec, gcol, z, zs, gdimg, gz, gabs),
                 mk_undefined(env));
}
FN(composite_backward_det_abs_workspace_bytes) { /* (totalPairs, numTiles, n, withDepth) -> bytes */
    ARGS(4); uint64_t pairs = (uint64_t)arg_number(&c, 0); uint32_t tiles = (uint32_t)arg_number(&c, 1), n = (uint32_t)arg_number(&c, 2);
    int depth = (int)arg_number(&c, 3); BAIL;
    return mk_number(env, (double)splat_composite_backward_det_abs_workspace_bytes(pairs, tiles, n, depth));
}
FN(composite_backward_det_abs) { /* composite_backward_det's arguments, then gradCenterAbs */
    ARGS(23); splat_ctx *x = arg_external(&c, 0); splat_composite_cfg cfg; fill_cfg(&c, 1, &cfg);
    void *col = arg_dptr(&c, 2); uint32_t cs = (uint32_t)arg_number(&c, 3); void *rec = arg_dptr(&c, 4), *proj = arg_dptr(&c, 5);
    void *idx = arg_dptr(&c, 6), *cnt = arg_dptr(&c, 7), *off = arg_dptr(&c, 8); uint64_t pairs = (uint64_t)arg_number(&c, 9);
    uint32_t w = (uint32_t)arg_number(&c, 10), h = (uint32_t)arg_number(&c, 11); void *gimg = arg_dptr(&c, 12);
    uint32_t n = (uint32_t)arg_number(&c, 13); void *grec = arg_dptr(&c, 14), *gcol = arg_dptr(&c, 15);
    void *z = arg_dptr(&c, 16); uint32_t zs = (uint32_t)arg_number(&c, 17); void *gdimg = arg_dptr(&c, 18), *gz = arg_dptr(&c, 19);
    void *ws = arg_dptr(&c, 20); uint64_t wb = (uint64_t)arg_number(&c, 21); void *gabs = arg_dptr(&c, 22); BAIL;
    return check(env, x, splat_composite_backward_det_abs(x, &cfg, col, cs, rec, proj, idx, cnt, off, pairs, w, h, gimg, n, grec, gcol, z, zs, gdimg,
                                                          gz, ws, wb, gabs), mk_undefined(env));
}
FN(composite_contribution) { /* (ctx, cfg[8], colorOpacity, cStride, records, indices, counts, offsets, W, H, pixelWeight|null, minWeight, n, hits|null, weightMax|null, weightSum|null) */
    ARGS(16); splat_ctx *x = arg_external(&c, 0); splat_composite_cfg cfg; fill_cfg(&c, 1, &cfg);
    void *col = arg_dptr(&c, 2); uint32_t cs = (uint32_t)arg_number(&c, 3); void *rec = arg_dptr(&c, 4);
    void *idx = arg_dptr(&c, 5), *cnt = arg_dptr(&c, 6), *off = arg_dptr(&c, 7);
    uint32_t w = (uint32_t)arg_number(&c, 8), h = (uint32_t)arg_number(&c, 9); void *pw = arg_dptr(&c, 10);
    float mw = (float)arg_number(&c, 11); uint32_t n = (uint32_t)arg_number(&c, 12);
    void *hits = arg_dptr(&c, 13), *wmax = arg_dptr(&c, 14), *wsum = arg_dptr(&c, 15); BAIL;
    return check(env, x, splat_composite_contribution(x, &cfg, col, cs, rec, idx, cnt, off, w, h, pw, mw, n, hits, wmax, wsum), mk_undefined(env));
}
FN(composite_features) { /* (ctx, cfg[8], colorOpacity, cStride, records, indices, counts, offsets, W, H, features, featureStrideFloats, channels, n, out) */
    ARGS(15); splat_ctx *x = arg_external(&c, 0); splat_composite_cfg cfg; fill_cfg(&c, 1, &cfg);
    void *col = arg_dptr(&c, 2); uint32_t cs = (uint32_t)arg_number(&c, 3); void *rec = arg_dptr(&c, 4);
    void *idx = arg_dptr(&c, 5), *cnt = arg_dptr(&c, 6), *off = arg_dptr(&c, 7);
    uint32_t w = (uint32_t)arg_number(&c, 8), h = (uint32_t)arg_number(&c, 9); void *f = arg_dptr(&c, 10);
    uint32_t fs = (uint32_t)arg_number(&c, 11), k = (uint32_t)arg_number(&c, 12), n = (uint32_t)arg_number(&c, 13);
    void *out = arg_dptr(&c, 14); BAIL;
    return check(env, x, splat_composite_features(x, &cfg, col, cs, rec, idx, cnt, off, w, h, f, fs, k, n, out), mk_undefined(env));
}
FN(composite_features_backward) { /* composite_features' arguments up to channels, then gradOut, n, gradRecords, gradColorOpacity, gradFeatures, gradFeatureStrideFloats */
    ARGS(19); splat_ctx *x = arg_external(&c, 0); splat_composite_cfg cfg; fill_cfg(&c, 1, &cfg);
    void *col = arg_dptr(&c, 2); uint32_t cs = (uint32_t)arg_number(&c, 3); void *rec = arg_dptr(&c, 4);
    void *idx = arg_dptr(&c, 5), *cnt = arg_dptr(&c, 6), *off = arg_dptr(&c, 7);
    uint32_t w = (uint32_t)arg_number(&c, 8), h = (uint32_t)arg_number(&c, 9); void *f = arg_dptr(&c, 10);
    uint32_t fs = (uint32_t)arg_number(&c, 11), k = (uint32_t)arg_number(&c, 12); void *gout = arg_dptr(&c, 13);
    uint32_t n = (uint32_t)arg_number(&c, 14); void *grec = arg_dptr(&c, 15), *gcol = arg_dptr(&c, 16), *gf = arg_dptr(&c, 17);
    uint32_t gfs = (uint32_t)arg_number(&c, 18); BAIL;
    return check(env, x, splat_composite_features_backward(x, &cfg, col, cs, rec, idx, cnt, off, w, h, f, fs, k, gout, n, grec, gcol, gf, gfs),
                 mk_undefined(env));
}
FN(project_ellipsoid_backward) { /* (ctx, Float32Array(22), positions, posStride, scales, scaleStride, rotations, rotStride, n, gradRecords, gradPositions, gradScales, gradRotations) */
    ARGS(13); splat_ctx *x = arg_external(&c, 0); size_t ub = 0; float *u = arg_hostbuf(&c, 1, &ub);
    void *pos = arg_dptr(&c, 2); uint32_t ps = (uint32_t)arg_number(&c, 3); void *scl = arg_dptr(&c, 4); uint32_t ss = (uint32_t)arg_number(&c, 5);
    void *rot = arg_dptr(&c, 6); uint32_t rs = (uint32_t)arg_number(&c, 7), n = (uint32_t)arg_number(&c, 8);
    void *grec = arg_dptr(&c, 9), *gp = arg_dptr(&c, 10), *gs = arg_dptr(&c, 11), *gr = arg_dptr(&c, 12); BAIL;
    if (ub < 22 * sizeof(float)) { napi_throw_range_error(env, NULL, "uniform block needs 22 floats"); return NULL; }
    return check(env, x, splat_project_ellipsoid_backward(x, u, pos, ps, scl, ss, rot, rs, n, grec, gp, gs, gr), mk_undefined(env));
}
FN(project_ellipsoid_backward_depth) { /* project_ellipsoid_backward's arguments, then gradDepth */
    ARGS(14); splat_ctx *x = arg_external(&c, 0); size_t ub = 0; float *u = arg_hostbuf(&c, 1, &ub);
    void *pos = arg_dptr(&c, 2); uint32_t ps = (uint32_t)arg_number(&c, 3); void *scl = arg_dptr(&c, 4); uint32_t ss = (uint32_t)arg_number(&c, 5);
    void *rot = arg_dptr(&c, 6); uint32_t rs = (uint32_t)arg_number(&c, 7), n = (uint32_t)arg_number(&c, 8);
    void *grec = arg_dptr(&c, 9), *gp = arg_dptr(&c, 10), *gs = arg_dptr(&c, 11), *gr = arg_dptr(&c, 12), *gz = arg_dptr(&c, 13); BAIL;
    if (ub < 22 * sizeof(float)) { napi_throw_range_error(env, NULL, "uniform block needs 22 floats"); return NULL; }
    return check(env, x, splat_project_ellipsoid_backward_depth(x, u, pos, ps, scl, ss, rot, rs, n, grec, gp, gs, gr, gz), mk_undefined(env));
}
FN(sh_colors_backward) { /* (ctx, Float32Array(3) eye, positions, posStride, sh, shStrideFloats, degree, opacity|null, gradColorOpacity, n, gradSh, gradPositions, gradOpacity) */
    ARGS(13); splat_ctx *x = arg_external(&c, 0); size_t eb = 0; float *eye = arg_hostbuf(&c, 1, &eb);
    void *pos = arg_dptr(&c, 2); uint32_t ps = (uint32_t)arg_number(&c, 3); void *sh = arg_dptr(&c, 4);
    uint32_t shs = (uint32_t)arg_number(&c, 5), deg = (uint32_t)arg_number(&c, 6); void *op = arg_dptr(&c, 7), *gcol = arg_dptr(&c, 8);
    uint32_t n = (uint32_t)arg_number(&c, 9); void *gsh = arg_dptr(&c, 10), *gp = arg_dptr(&c, 11), *gop = arg_dptr(&c, 12); BAIL;
    if (eb < 3 * sizeof(float)) { napi_throw_range_error(env, NULL, "eye needs 3 floats"); return NULL; }
    return check(env, x, splat_sh_colors_backward(x, eye, pos, ps, sh, shs, deg, op, gcol, n, gsh, gp, gop), mk_undefined(env));
}
FN(project_ellipsoid_backward_camera) { /* project_ellipsoid_backward's arguments, then gradDepth|null, gradUniforms (device, 22 floats) */
    ARGS(15); splat_ctx *x = arg_external(&c, 0); size_t ub = 0; float *u = arg_hostbuf(&c, 1, &ub);
    void *pos = arg_dptr(&c, 2); uint32_t ps = (uint32_t)arg_number(&c, 3); void *scl = arg_dptr(&c, 4); uint32_t ss = (uint32_t)arg_number(&c, 5);
    void *rot = arg_dptr(&c, 6); uint32_t rs = (uint32_t)arg_number(&c, 7), n = (uint32_t)arg_number(&c, 8);
    void *grec = arg_dptr(&c, 9), *gp = arg_dptr(&c, 10), *gs = arg_dptr(&c, 11), *gr = arg_dptr(&c, 12), *gz = arg_dptr(&c, 13);
    void *gu = arg_dptr(&c, 14); BAIL;
    if (ub < 22 * sizeof(float)) { napi_throw_range_error(env, NULL, "uniform block needs 22 floats"); return NULL; }
    return check(env, x, splat_project_ellipsoid_backward_camera(x, u, pos, ps, scl, ss, rot, rs, n, grec, gp, gs, gr, gz, gu), mk_undefined(env));
}
FN(project_ellipsoid_backward_aa) { /* project_ellipsoid_backward's arguments, then gradDepth|null, gradUniforms|null (device, 22 floats), gradRho */
    ARGS(16); splat_ctx *x = arg_external(&c, 0); size_t ub = 0; float *u = arg_hostbuf(&c, 1, &ub);
    void *pos = arg_dptr(&c, 2); uint32_t ps = (uint32_t)arg_number(&c, 3); void *scl = arg_dptr(&c, 4); uint32_t ss = (uint32_t)arg_number(&c, 5);
    void *rot = arg_dptr(&c, 6); uint32_t rs = (uint32_t)arg_number(&c, 7), n = (uint32_t)arg_number(&c, 8);
    void *grec = arg_dptr(&c, 9), *gp = arg_dptr(&c, 10), *gs = arg_dptr(&c, 11), *gr = arg_dptr(&c, 12), *gz = arg_dptr(&c, 13);
    void *gu = arg_dptr(&c, 14), *grho = arg_dptr(&c, 15); BAIL;
    if (ub < 22 * sizeof(float)) { napi_throw_range_error(env, NULL, "uniform block needs 22 floats"); return NULL; }
    return check(env, x, splat_project_ellipsoid_backward_aa(x, u, pos, ps, scl, ss, rot, rs, n, grec, gp, gs, gr, gz, gu, grho), mk_undefined(env));
}
FN(sh_colors_backward_camera) { /* sh_colors_backward's arguments, then gradEye (device, 4 floats) */
    ARGS(14); splat_ctx *x = arg_external(&c, 0); size_t eb = 0; float *eye = arg_hostbuf(&c, 1, &eb);
    void *pos = arg_dptr(&c, 2); uint32_t ps = (uint32_t)arg_number(&c, 3); void *sh = arg_dptr(&c, 4);
    uint32_t shs = (uint32_t)arg_number(&c, 5), deg = (uint32_t)arg_number(&c, 6); void *op = arg_dptr(&c, 7), *gcol = arg_dptr(&c, 8);
    uint32_t n = (uint32_t)arg_number(&c, 9); void *gsh = arg_dptr(&c, 10), *gp = arg_dptr(&c, 11), *gop = arg_dptr(&c, 12);
    void *ge = arg_dptr(&c, 13); BAIL;
    if (eb < 3 * sizeof(float)) { napi_throw_range_error(env, NULL, "eye needs 3 floats"); return NULL; }
    return check(env, x, splat_sh_colors_backward_camera(x, eye, pos, ps, sh, shs, deg, op, gcol, n, gsh, gp, gop, ge), mk_undefined(env));
}
FN(image_loss_workspace_bytes) { /* (W, H) -> bytes */
    ARGS(2); uint32_t w = (uint32_t)arg_number(&c, 0), h = (uint32_t)arg_number(&c, 1); BAIL;
    return mk_number(env, (double)splat_image_loss_workspace_bytes(w, h));
}
FN(image_loss) { /* (ctx, image, imageStride, target, targetStride, W, H, lambda, workspace|null, workspaceBytes, out4 (device: loss, l1, ssim, 0)) */
    ARGS(11); splat_ctx *x = arg_external(&c, 0); void *img = arg_dptr(&c, 1); uint32_t is = (uint32_t)arg_number(&c, 2);
    void *tgt = arg_dptr(&c, 3); uint32_t ts = (uint32_t)arg_number(&c, 4), w = (uint32_t)arg_number(&c, 5), h = (uint32_t)arg_number(&c, 6);
    float lambda = (float)arg_number(&c, 7); void *ws = arg_dptr(&c, 8); uint64_t wb = (uint64_t)arg_number(&c, 9); void *out = arg_dptr(&c, 10); BAIL;
    return check(env, x, splat_image_loss(x, img, is, tgt, ts, w, h, lambda, ws, wb, out), mk_undefined(env));
}
FN(image_loss_backward) { /* image_loss's arguments up to workspaceBytes, then upstream (device, 1 float), gradImage, gradStride */
    ARGS(13); splat_ctx *x = arg_external(&c, 0); void *img = arg_dptr(&c, 1); uint32_t is = (uint32_t)arg_number(&c, 2);
    void *tgt = arg_dptr(&c, 3); uint32_t ts = (uint32_t)arg_number(&c, 4), w = (uint32_t)arg_number(&c, 5), h = (uint32_t)arg_number(&c, 6);
    float lambda = (float)arg_number(&c, 7); void *ws = arg_dptr(&c, 8); uint64_t wb = (uint64_t)arg_number(&c, 9);
    void *up = arg_dptr(&c, 10), *g = arg_dptr(&c, 11); uint32_t gs = (uint32_t)arg_number(&c, 12); BAIL;
    return check(env, x, splat_image_loss_backward(x, img, is, tgt, ts, w, h, lambda, ws, wb, up, g, gs), mk_undefined(env));
}
FN(camera_rays) { /* (Float32Array(22)) -> [D0 (3), Dx (3), Dy (3), sigma]: host only, no ctx */
    ARGS(1); size_t ub = 0; float *u = arg_hostbuf(&c, 0, &ub); BAIL;
    if (ub < 22 * sizeof(float)) { napi_throw_range_error(env, NULL, "uniform block needs 22 floats"); return NULL; }
    double out[10];
    int rc = splat_camera_rays(u, out);
    if (rc != SPLAT_OK) return check(env, NULL, rc, NULL);
    napi_value arr;
    if (napi_create_array_with_length(env, 10, &arr) != napi_ok) return NULL;
    for (uint32_t i = 0; i < 10; ++i) napi_set_element(env, arr, i, mk_number(env, out[i]));
    return arr;
}
FN(depth_normals) { /* (ctx, Float32Array(22), depthKind (0 distance | 1 z), depth, W, H, normals, normalStride) */
    ARGS(8); splat_ctx *x = arg_external(&c, 0); size_t ub = 0; float *u = arg_hostbuf(&c, 1, &ub); uint32_t kind = (uint32_t)arg_number(&c, 2);
    void *z = arg_dptr(&c, 3); uint32_t w = (uint32_t)arg_number(&c, 4), h = (uint32_t)arg_number(&c, 5);
    void *nm = arg_dptr(&c, 6); uint32_t ns = (uint32_t)arg_number(&c, 7); BAIL;
    if (ub < 22 * sizeof(float)) { napi_throw_range_error(env, NULL, "uniform block needs 22 floats"); return NULL; }
    return check(env, x, splat_depth_normals(x, u, kind, z, w, h, nm, ns), mk_undefined(env));
}
FN(depth_normals_backward) { /* (ctx, Float32Array(22), depthKind, depth, W, H, gradNormals, gradStride, gradDepth) */
    ARGS(9); splat_ctx *x = arg_external(&c, 0); size_t ub = 0; float *u = arg_hostbuf(&c, 1, &ub); uint32_t kind = (uint32_t)arg_number(&c, 2);
    void *z = arg_dptr(&c, 3); uint32_t w = (uint32_t)arg_number(&c, 4), h = (uint32_t)arg_number(&c, 5);
    void *gn = arg_dptr(&c, 6); uint32_t gs = (uint32_t)arg_number(&c, 7); void *gz = arg_dptr(&c, 8); BAIL;
    if (ub < 22 * sizeof(float)) { napi_throw_range_error(env, NULL, "uniform block needs 22 floats"); return NULL; }
    return check(env, x, splat_depth_normals_backward(x, u, kind, z, w, h, gn, gs, gz), mk_undefined(env));
}
FN(normal_consistency) { /* (ctx, Float32Array(22), depthKind, depth, normalMap, mapStride, weight|null, W, H, out4 (device: loss, valid fraction, 0, 0)) */
    ARGS(10); splat_ctx *x = arg_external(&c, 0); size_t ub = 0; float *u = arg_hostbuf(&c, 1, &ub); uint32_t kind = (uint32_t)arg_number(&c, 2);
    void *z = arg_dptr(&c, 3), *nm = arg_dptr(&c, 4); uint32_t ms = (uint32_t)arg_number(&c, 5); void *wt = arg_dptr(&c, 6);
    uint32_t w = (uint32_t)arg_number(&c, 7), h = (uint32_t)arg_number(&c, 8); void *out = arg_dptr(&c, 9); BAIL;
    if (ub < 22 * sizeof(float)) { napi_throw_range_error(env, NULL, "uniform block needs 22 floats"); return NULL; }
    return check(env, x, splat_normal_consistency(x, u, kind, z, nm, ms, wt, w, h, out), mk_undefined(env));
}
FN(normal_consistency_backward) { /* normal_consistency's arguments up to H, then upstream (device, 1 float), gradMap, gradMapStride, gradDepth */
    ARGS(13); splat_ctx *x = arg_external(&c, 0); size_t ub = 0; float *u = arg_hostbuf(&c, 1, &ub); uint32_t kind = (uint32_t)arg_number(&c, 2);
    void *z = arg_dptr(&c, 3), *nm = arg_dptr(&c, 4); uint32_t ms = (uint32_t)arg_number(&c, 5); void *wt = arg_dptr(&c, 6);
    uint32_t w = (uint32_t)arg_number(&c, 7), h = (uint32_t)arg_number(&c, 8); void *up = arg_dptr(&c, 9), *gm = arg_dptr(&c, 10);
    uint32_t gms = (uint32_t)arg_number(&c, 11); void *gz = arg_dptr(&c, 12); BAIL;
    if (ub < 22 * sizeof(float)) { napi_throw_range_error(env, NULL, "uniform block needs 22 floats"); return NULL; }
    return check(env, x, splat_normal_consistency_backward(x, u, kind, z, nm, ms, wt, w, h, up, gm, gms, gz), mk_undefined(env));
}
static void fill_tsdf_grid(call_t *c, size_t i, splat_tsdf_grid *g) { /* [originX, originY, originZ, voxel, nx, ny, nz, trunc] */
    memset(g, 0, sizeof *g);
    double v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool is = false;
    napi_is_array(c->env, c->argv[i], &is);
    if (!is) { c->failed = 1; napi_throw_type_error(c->env, NULL, "expected the TSDF grid as an array of 8 numbers"); return; }
    for (uint32_t k = 0; k < 8; ++k) {
        napi_value e;
        double d;
        if (napi_get_element(c->env, c->argv[i], k, &e) == napi_ok && napi_get_value_double(c->env, e, &d) == napi_ok) v[k] = d;
    }
    g->origin[0] = (float)v[0]; g->origin[1] = (float)v[1]; g->origin[2] = (float)v[2]; g->voxel = (float)v[3];
    g->dims[0] = (uint32_t)v[4]; g->dims[1] = (uint32_t)v[5]; g->dims[2] = (uint32_t)v[6]; g->trunc = (float)v[7];
}
FN(tsdf_integrate) { /* (ctx, grid[8], tsdf, weight, color|null, Float32Array(22), depthKind, depth, obsWeight|null, image|null, imageStride, W, H, maxWeight) */
    ARGS(14); splat_ctx *x = arg_external(&c, 0); splat_tsdf_grid g; fill_tsdf_grid(&c, 1, &g);
    void *td = arg_dptr(&c, 2), *wt = arg_dptr(&c, 3), *col = arg_dptr(&c, 4); size_t ub = 0; float *u = arg_hostbuf(&c, 5, &ub);
    uint32_t kind = (uint32_t)arg_number(&c, 6); void *z = arg_dptr(&c, 7), *ow = arg_dptr(&c, 8), *img = arg_dptr(&c, 9);
    uint32_t is = (uint32_t)arg_number(&c, 10), w = (uint32_t)arg_number(&c, 11), h = (uint32_t)arg_number(&c, 12); float mw = (float)arg_number(&c, 13); BAIL;
    if (ub < 22 * sizeof(float)) { napi_throw_range_error(env, NULL, "uniform block needs 22 floats"); return NULL; }
    return check(env, x, splat_tsdf_integrate(x, &g, td, wt, col, u, kind, z, ow, img, is, w, h, mw), mk_undefined(env));
}
FN(tsdf_mesh_workspace_bytes) { /* (nx, ny, nz) -> bytes */
    ARGS(3); uint32_t nx = (uint32_t)arg_number(&c, 0), ny = (uint32_t)arg_number(&c, 1), nz = (uint32_t)arg_number(&c, 2); BAIL;
    return mk_number(env, (double)splat_tsdf_mesh_workspace_bytes(nx, ny, nz));
}
FN(tsdf_mesh_count) { /* (ctx, grid[8], tsdf, weight, minWeight, workspace, workspaceBytes) -> [vertices, triangles] (waits) */
    ARGS(7); splat_ctx *x = arg_external(&c, 0); splat_tsdf_grid g; fill_tsdf_grid(&c, 1, &g);
    void *td = arg_dptr(&c, 2), *wt = arg_dptr(&c, 3); float mw = (float)arg_number(&c, 4); void *ws = arg_dptr(&c, 5);
    uint64_t wb = (uint64_t)arg_number(&c, 6); BAIL;
    uint32_t counts[2] = {0, 0};
    int rc = splat_tsdf_mesh_count(x, &g, td, wt, mw, ws, wb, &counts[0], &counts[1]);
    if (rc != SPLAT_OK) return check(env, x, rc, NULL);
    napi_value arr;
    if (napi_create_array_with_length(env, 2, &arr) != napi_ok) return NULL;
    for (uint32_t k = 0; k < 2; ++k) napi_set_element(env, arr, k, mk_number(env, (double)counts[k]));
    return arr;
}
FN(tsdf_mesh_emit) { /* (ctx, grid[8], tsdf, color|null, workspace, workspaceBytes, vertices, vertexColors|null, triangles) */
    ARGS(9); splat_ctx *x = arg_external(&c, 0); splat_tsdf_grid g; fill_tsdf_grid(&c, 1, &g);
    void *td = arg_dptr(&c, 2), *col = arg_dptr(&c, 3), *ws = arg_dptr(&c, 4); uint64_t wb = (uint64_t)arg_number(&c, 5);
    void *vx = arg_dptr(&c, 6), *vc = arg_dptr(&c, 7), *tr = arg_dptr(&c, 8); BAIL;
    return check(env, x, splat_tsdf_mesh_emit(x, &g, td, col, ws, wb, vx, vc, tr), mk_undefined(env));
}
/* splat_densify_cfg from [gradThreshold, scaleThreshold, minOpacity, maxScreenRadius, maxWorldScale, maxSplats, seed (integer < 2^53)] */
static void fill_densify_cfg(call_t *c, size_t i, splat_densify_cfg *cfg) {
    memset(cfg, 0, sizeof *cfg);
    double v[7] = {0, 0, 0, 0, 0, 0, 0};
    bool is = false;
    napi_is_array(c->env, c->argv[i], &is);
    if (!is) { c->failed = 1; napi_throw_type_error(c->env, NULL, "expected the densify config as an array of 7 numbers"); return; }
    for (uint32_t k = 0; k < 7; ++k) {
        napi_value e;
        double d;
        if (napi_get_element(c->env, c->argv[i], k, &e) == napi_ok && napi_get_value_double(c->env, e, &d) == napi_ok) v[k] = d;
    }
    cfg->grad_threshold = (float)v[0]; cfg->scale_threshold = (float)v[1]; cfg->min_opacity = (float)v[2];
    cfg->max_screen_radius = (float)v[3]; cfg->max_world_scale = (float)v[4]; cfg->max_splats = (uint32_t)v[5]; cfg->seed = (uint64_t)v[6];
}
FN(adam_step) { /* (ctx, param, grad, m, v, rows, floatsPerRow, headFloats, stepHead, stepTail, beta1, beta2, invSqrtBc2, eps, visible|null) */
    ARGS(15); splat_ctx *x = arg_external(&c, 0); void *p = arg_dptr(&c, 1), *g = arg_dptr(&c, 2), *m = arg_dptr(&c, 3), *v = arg_dptr(&c, 4);
    uint32_t rows = (uint32_t)arg_number(&c, 5), fpr = (uint32_t)arg_number(&c, 6), head = (uint32_t)arg_number(&c, 7);
    double sh = arg_number(&c, 8), st = arg_number(&c, 9), b1 = arg_number(&c, 10), b2 = arg_number(&c, 11), bc = arg_number(&c, 12);
    double eps = arg_number(&c, 13); void *vis = arg_dptr(&c, 14); BAIL;
    return check(env, x, splat_adam_step(x, p, g, m, v, rows, fpr, head, sh, st, b1, b2, bc, eps, vis), mk_undefined(env));
}
typedef int (*density_accumulate_fn)(splat_ctx *, const void *, const void *, uint32_t, uint32_t, uint32_t, void *, void *, void *, void *);
static napi_value density_accumulate_call(napi_env env, napi_callback_info info, density_accumulate_fn accumulate) {
    ARGS(10); splat_ctx *x = arg_external(&c, 0); void *rec = arg_dptr(&c, 1), *gr = arg_dptr(&c, 2);
    uint32_t n = (uint32_t)arg_number(&c, 3), w = (uint32_t)arg_number(&c, 4), h = (uint32_t)arg_number(&c, 5);
    void *ga = arg_dptr(&c, 6), *dn = arg_dptr(&c, 7), *mr = arg_dptr(&c, 8), *vis = arg_dptr(&c, 9); BAIL;
    return check(env, x, accumulate(x, rec, gr, n, w, h, ga, dn, mr, vis), mk_undefined(env));
}
/* (ctx, records, gradRecords, n, W, H, gradAccum, denom, maxRadius, visible); _abs: gradCenterAbs (n x 2) for gradRecords; _surfel: surfel records */
FN(density_accumulate) { return density_accumulate_call(env, info, splat_density_accumulate); }
FN(density_accumulate_abs) { return density_accumulate_call(env, info, splat_density_accumulate_abs); }
FN(density_accumulate_surfel) { return density_accumulate_call(env, info, splat_density_accumulate_surfel); }
FN(densify_plan_workspace_bytes) { /* (n) -> bytes */
    ARGS(1); uint32_t n = (uint32_t)arg_number(&c, 0); BAIL;
    return mk_number(env, (double)splat_densify_plan_workspace_bytes(n));
}
typedef int (*densify_plan_fn)(splat_ctx *, const void *, const void *, const void *, const void *, const void *, uint32_t,
                               const splat_densify_cfg *, void *, uint64_t, void *, uint32_t *, uint32_t *);
static napi_value densify_plan_call(napi_env env, napi_callback_info info, densify_plan_fn plan) {
    ARGS(11); splat_ctx *x = arg_external(&c, 0); void *ls = arg_dptr(&c, 1), *ol = arg_dptr(&c, 2), *ga = arg_dptr(&c, 3), *dn = arg_dptr(&c, 4);
    void *mr = arg_dptr(&c, 5); uint32_t n = (uint32_t)arg_number(&c, 6); splat_densify_cfg cfg; fill_densify_cfg(&c, 7, &cfg);
    void *ws = arg_dptr(&c, 8); uint64_t wb = (uint64_t)arg_number(&c, 9); void *rows = arg_dptr(&c, 10); BAIL;
    uint32_t n_out = 0, counts[4] = {0, 0, 0, 0};
    int rc = plan(x, ls, ol, ga, dn, mr, n, &cfg, ws, wb, rows, &n_out, counts);
    if (rc != SPLAT_OK) return check(env, x, rc, NULL);
    napi_value arr;
    if (napi_create_array_with_length(env, 5, &arr) != napi_ok) return NULL;
    napi_set_element(env, arr, 0, mk_number(env, n_out));
    for (uint32_t k = 0; k < 4; ++k) napi_set_element(env, arr, k + 1, mk_number(env, counts[k]));
    return arr;
}
/* (ctx, logScales, opacityLogits, gradAccum, denom, maxRadius, n, cfg[7], workspace, workspaceBytes, rows) -> [nOut, pruned, kept, cloned, split] (waits) */
FN(densify_plan) { return densify_plan_call(env, info, splat_densify_plan); }
FN(densify_plan_surfel) { return densify_plan_call(env, info, splat_densify_plan_surfel); } /* logScales: n x 2 */
typedef int (*densify_geometry_fn)(splat_ctx *, const void *, uint32_t, const void *, const void *, const void *, const splat_densify_cfg *,
                                   void *, void *);
static napi_value densify_geometry_call(napi_env env, napi_callback_info info, densify_geometry_fn geometry) {
    ARGS(9); splat_ctx *x = arg_external(&c, 0); void *rows = arg_dptr(&c, 1); uint32_t n = (uint32_t)arg_number(&c, 2);
    void *mu = arg_dptr(&c, 3), *ls = arg_dptr(&c, 4), *rot = arg_dptr(&c, 5); splat_densify_cfg cfg; fill_densify_cfg(&c, 6, &cfg);
    void *mo = arg_dptr(&c, 7), *lo = arg_dptr(&c, 8); BAIL;
    return check(env, x, geometry(x, rows, n, mu, ls, rot, &cfg, mo, lo), mk_undefined(env));
}
/* (ctx, rows, nOut, means, logScales, rotations, cfg[7], meansOut, logScalesOut); _surfel: logScales n x 2, logScalesOut nOut x 2 */
FN(densify_geometry) { return densify_geometry_call(env, info, splat_densify_geometry); }
FN(densify_geometry_surfel) { return densify_geometry_call(env, info, splat_densify_geometry_surfel); }
FN(densify_rows) { /* (ctx, rows, nOut, in, out, floatsPerRow, mode: 0 copy, 1 zero the new rows) */
    ARGS(7); splat_ctx *x = arg_external(&c, 0); void *rows = arg_dptr(&c, 1); uint32_t n = (uint32_t)arg_number(&c, 2);
    void *in = arg_dptr(&c, 3), *out = arg_dptr(&c, 4); uint32_t fpr = (uint32_t)arg_number(&c, 5), mode = (uint32_t)arg_number(&c, 6); BAIL;
    return check(env, x, splat_densify_rows(x, rows, n, in, out, fpr, mode), mk_undefined(env));
}
FN(mcmc_sample_workspace_bytes) { /* (n) -> bytes */
    ARGS(1); uint32_t n = (uint32_t)arg_number(&c, 0); BAIL;
    return mk_number(env, (double)splat_mcmc_sample_workspace_bytes(n));
}
FN(mcmc_sample) { /* (ctx, opacityLogits, n, mode: 1 relocate, 2 add, nDraws, minOpacity, seed (integer < 2^53), workspace, workspaceBytes, targets, sources, counts) -> [dead, alive, draws] (waits) */
    ARGS(12); splat_ctx *x = arg_external(&c, 0); void *ol = arg_dptr(&c, 1); uint32_t n = (uint32_t)arg_number(&c, 2);
    uint32_t mode = (uint32_t)arg_number(&c, 3), nd = (uint32_t)arg_number(&c, 4); double mo = arg_number(&c, 5);
    uint64_t seed = (uint64_t)arg_number(&c, 6); void *ws = arg_dptr(&c, 7); uint64_t wb = (uint64_t)arg_number(&c, 8);
    void *tg = arg_dptr(&c, 9), *sr = arg_dptr(&c, 10), *ct = arg_dptr(&c, 11); BAIL;
    uint32_t words[3] = {0, 0, 0};
    int rc = splat_mcmc_sample(x, ol, n, mode, nd, mo, seed, ws, wb, tg, sr, ct, words);
    if (rc != SPLAT_OK) return check(env, x, rc, NULL);
    napi_value arr;
    if (napi_create_array_with_length(env, 3, &arr) != napi_ok) return NULL;
    for (uint32_t k = 0; k < 3; ++k) napi_set_element(env, arr, k, mk_number(env, (double)words[k]));
    return arr;
}
FN(mcmc_apply) { /* (ctx, targets, sources, counts, n, nDraws, rows, minOpacity, planes[15]: 5 parameters, 5 m, 5 v (device pointers or null), shFloats) */
    ARGS(10); splat_ctx *x = arg_external(&c, 0); void *tg = arg_dptr(&c, 1), *sr = arg_dptr(&c, 2), *ct = arg_dptr(&c, 3);
    uint32_t n = (uint32_t)arg_number(&c, 4), nd = (uint32_t)arg_number(&c, 5), rows = (uint32_t)arg_number(&c, 6); double mo = arg_number(&c, 7);
    splat_mcmc_planes pl; memset(&pl, 0, sizeof pl);
    bool is = false; uint32_t len = 0;
    napi_is_array(env, c.argv[8], &is);
    if (is) napi_get_array_length(env, c.argv[8], &len);
    if (!is || len != 15) { napi_throw_type_error(env, NULL, "expected the planes as an array of 15 device pointers"); return NULL; }
    for (uint32_t k = 0; k < 15; ++k) {
        napi_value e; napi_valuetype t; double d = 0;
        napi_get_element(env, c.argv[8], k, &e);
        napi_typeof(env, e, &t);
        if (t != napi_null && t != napi_undefined && napi_get_value_double(env, e, &d) != napi_ok) {
            napi_throw_type_error(env, NULL, "expected the planes as an array of 15 device pointers"); return NULL;
        }
        void *p = (void *)(uintptr_t)d;
        if (k < 5) pl.param[k] = p; else if (k < 10) pl.m[k - 5] = p; else pl.v[k - 10] = p;
    }
    pl.sh_floats = (uint32_t)arg_number(&c, 9); BAIL;
    return check(env, x, splat_mcmc_apply(x, tg, sr, ct, n, nd, rows, mo, &pl), mk_undefined(env));
}
FN(mcmc_noise) { /* (ctx, means, logScales, rotations, opacityLogits, n, scale, step, seed (integer < 2^53)) */
    ARGS(9); splat_ctx *x = arg_external(&c, 0); void *mu = arg_dptr(&c, 1), *ls = arg_dptr(&c, 2), *rot = arg_dptr(&c, 3), *ol = arg_dptr(&c, 4);
    uint32_t n = (uint32_t)arg_number(&c, 5); double scale = arg_number(&c, 6); uint32_t step = (uint32_t)arg_number(&c, 7);
    uint64_t seed = (uint64_t)arg_number(&c, 8); BAIL;
    return check(env, x, splat_mcmc_noise(x, mu, ls, rot, ol, n, scale, step, seed), mk_undefined(env));
}
FN(knn_workspace_bytes) { /* (n) -> bytes */
    ARGS(1); uint32_t n = (uint32_t)arg_number(&c, 0); BAIL;
    return mk_number(env, (double)splat_knn_workspace_bytes(n));
}
FN(knn_mean_sq) { /* (ctx, sorter, points, strideFloats, n, workspace, workspaceBytes, meanSq, evaluations|null) */
    ARGS(9); splat_ctx *x = arg_external(&c, 0); splat_sorter *s = arg_external(&c, 1); void *pts = arg_dptr(&c, 2);
    uint32_t stride = (uint32_t)arg_number(&c, 3), n = (uint32_t)arg_number(&c, 4); void *ws = arg_dptr(&c, 5);
    uint64_t wb = (uint64_t)arg_number(&c, 6); void *out = arg_dptr(&c, 7), *ev = arg_dptr(&c, 8); BAIL;
    return check(env, x, splat_knn_mean_sq(x, s, pts, stride, n, ws, wb, out, ev), mk_undefined(env));
}
FN(render_frame_ellipsoids) { /* (ctx, sorter, binner, cfg[8], Float32Array(22), positions, scales, rotations, colorOpacity, n, W, H, projected|null, out8|null, outF|null, [depth, alpha, ids]|null) */
    ARGS(16); splat_ctx *x = arg_external(&c, 0); splat_sorter *s = arg_external(&c, 1); splat_binner *b = arg_external(&c, 2);
    splat_composite_cfg cfg; fill_cfg(&c, 3, &cfg); size_t ub = 0; float *u = arg_hostbuf(&c, 4, &ub);
    void *pos = arg_dptr(&c, 5), *scl = arg_dptr(&c, 6), *rot = arg_dptr(&c, 7), *co = arg_dptr(&c, 8);
    uint32_t n = (uint32_t)arg_number(&c, 9), w = (uint32_t)arg_number(&c, 10), h = (uint32_t)arg_number(&c, 11);
    void *proj = arg_dptr(&c, 12), *o8 = arg_dptr(&c, 13), *of = arg_dptr(&c, 14); BAIL;
    splat_aov a; const splat_aov *ap = fill_aov(&c, 15, &a);
    if (ub < 22 * sizeof(float)) { napi_throw_range_error(env, NULL, "uniform block needs 22 floats"); return NULL; }
    int rc = splat_render_frame_ellipsoids(x, s, b, &cfg, u, pos, scl, rot, co, n, w, h, proj, o8, of, ap);
    if (AGAIN(rc)) rc = splat_render_frame_ellipsoids(x, s, b, &cfg, u, pos, scl, rot, co, n, w, h, proj, o8, of, ap);
    return check(env, x, rc, mk_undefined(env));
}
FN(render_frame_ellipsoids_aa) { /* render_frame_ellipsoids' arguments: the antialiased frame */
    ARGS(16); splat_ctx *x = arg_external(&c, 0); splat_sorter *s = arg_external(&c, 1); splat_binner *b = arg_external(&c, 2);
    splat_composite_cfg cfg; fill_cfg(&c, 3, &cfg); size_t ub = 0; float *u = arg_hostbuf(&c, 4, &ub);
    void *pos = arg_dptr(&c, 5), *scl = arg_dptr(&c, 6), *rot = arg_dptr(&c, 7), *co = arg_dptr(&c, 8);
    uint32_t n = (uint32_t)arg_number(&c, 9), w = (uint32_t)arg_number(&c, 10), h = (uint32_t)arg_number(&c, 11);
    void *proj = arg_dptr(&c, 12), *o8 = arg_dptr(&c, 13), *of = arg_dptr(&c, 14); BAIL;
    splat_aov a; const splat_aov *ap = fill_aov(&c, 15, &a);
    if (ub < 22 * sizeof(float)) { napi_throw_range_error(env, NULL, "uniform block needs 22 floats"); return NULL; }
    int rc = splat_render_frame_ellipsoids_aa(x, s, b, &cfg, u, pos, scl, rot, co, n, w, h, proj, o8, of, ap);
    if (AGAIN(rc)) rc = splat_render_frame_ellipsoids_aa(x, s, b, &cfg, u, pos, scl, rot, co, n, w, h, proj, o8, of, ap);
    return check(env, x, rc, mk_undefined(env));
}
FN(render_frame) { /* (ctx, sorter, binner, cfg[5], Float32Array(22), props, normals, n, W, H, projected, out8|null, outF|null) */
    ARGS(13); splat_ctx *x = arg_external(&c, 0); splat_sorter *s = arg_external(&c, 1); splat_binner *b = arg_external(&c, 2);
    splat_composite_cfg cfg; fill_cfg(&c, 3, &cfg); size_t ub = 0; float *u = arg_hostbuf(&c, 4, &ub);
    void *props = arg_dptr(&c, 5), *nrm = arg_dptr(&c, 6); uint32_t n = (uint32_t)arg_number(&c, 7), w = (uint32_t)arg_number(&c, 8), h = (uint32_t)arg_number(&c, 9);
    void *proj = arg_dptr(&c, 10), *o8 = arg_dptr(&c, 11), *of = arg_dptr(&c, 12); BAIL;
    if (ub < 22 * sizeof(float)) { napi_throw_range_error(env, NULL, "uniform block needs 22 floats"); return NULL; }
    int rc = splat_render_frame(x, s, b, &cfg, u, props, nrm, n, w, h, proj, o8, of);
    if (AGAIN(rc)) rc = splat_render_frame(x, s, b, &cfg, u, props, nrm, n, w, h, proj, o8, of);
    return check(env, x, rc, mk_undefined(env));
}

FN(render_frame_planes) { /* (ctx, sorter, binner, cfg[5], Float32Array(22), posRadius, colorOpacity, normals, n, W, H, projected, out8|null, outF|null) */
    ARGS(14); splat_ctx *x = arg_external(&c, 0); splat_sorter *s = arg_external(&c, 1); splat_binner *b = arg_external(&c, 2);
    splat_composite_cfg cfg; fill_cfg(&c, 3, &cfg); size_t ub = 0; float *u = arg_hostbuf(&c, 4, &ub);
    void *pr = arg_dptr(&c, 5), *co = arg_dptr(&c, 6), *nrm = arg_dptr(&c, 7);
    uint32_t n = (uint32_t)arg_number(&c, 8), w = (uint32_t)arg_number(&c, 9), h = (uint32_t)arg_number(&c, 10);
    void *proj = arg_dptr(&c, 11), *o8 = arg_dptr(&c, 12), *of = arg_dptr(&c, 13); BAIL;
    if (ub < 22 * sizeof(float)) { napi_throw_range_error(env, NULL, "uniform block needs 22 floats"); return NULL; }
    int rc = splat_render_frame_planes(x, s, b, &cfg, u, pr, co, nrm, n, w, h, proj, o8, of);
    if (AGAIN(rc)) rc = splat_render_frame_planes(x, s, b, &cfg, u, pr, co, nrm, n, w, h, proj, o8, of);
    return check(env, x, rc, mk_undefined(env));
}

/* ---- SDF splat generation (include/splat.h: "SDF splat generation") ---- */
static int sdf_program(call_t *c, size_t i, splat_sdf_instr *prog, uint32_t *count) { /* Float32Array of 8 floats per instruction: [op, a0..a6] */
    size_t nb = 0; float *f = arg_hostbuf(c, i, &nb);
    if (c->failed) return 0;
    size_t n = nb / (8 * sizeof(float));
    if (n > SPLAT_SDF_MAX_INSTR) { c->failed = 1; napi_throw_range_error(c->env, NULL, "SDF program: too many instructions"); return 0; }
    for (size_t k = 0; k < n; k++) { prog[k].op = (uint32_t)f[k * 8]; for (int j = 0; j < 7; j++) prog[k].a[j] = f[k * 8 + 1 + j]; }
    *count = (uint32_t)n;
    return 1;
}
FN(sdf_gradients) { /* (ctx, program, positions, n, gradients) */
    ARGS(5); splat_ctx *x = arg_external(&c, 0); splat_sdf_instr prog[SPLAT_SDF_MAX_INSTR]; uint32_t cnt = 0;
    if (!sdf_program(&c, 1, prog, &cnt)) return NULL;
    void *pos = arg_dptr(&c, 2); uint32_t n = (uint32_t)arg_number(&c, 3); void *g = arg_dptr(&c, 4); BAIL;
    return check(env, x, splat_sdf_gradients(x, prog, cnt, pos, n, g), mk_undefined(env));
}
FN(sdf_update_positions) { /* (ctx, positions, gradients, n, nextPositions) */
    ARGS(5); splat_ctx *x = arg_external(&c, 0); void *pos = arg_dptr(&c, 1), *g = arg_dptr(&c, 2); uint32_t n = (uint32_t)arg_number(&c, 3);
    void *nx = arg_dptr(&c, 4); BAIL;
    return check(env, x, splat_sdf_update_positions(x, pos, g, n, nx), mk_undefined(env));
}
FN(sdf_scale_factors) { /* (ctx, program, positions, n, scaleFactors) */
    ARGS(5); splat_ctx *x = arg_external(&c, 0); splat_sdf_instr prog[SPLAT_SDF_MAX_INSTR]; uint32_t cnt = 0;
    if (!sdf_program(&c, 1, prog, &cnt)) return NULL;
    void *pos = arg_dptr(&c, 2); uint32_t n = (uint32_t)arg_number(&c, 3); void *sf = arg_dptr(&c, 4); BAIL;
    return check(env, x, splat_sdf_scale_factors(x, prog, cnt, pos, n, sf), mk_undefined(env));
}
FN(sdf_curvature) { /* (ctx, gradients, scaleFactors, n, curvature) */
    ARGS(5); splat_ctx *x = arg_external(&c, 0); void *g = arg_dptr(&c, 1), *sf = arg_dptr(&c, 2); uint32_t n = (uint32_t)arg_number(&c, 3);
    void *cur = arg_dptr(&c, 4); BAIL;
    return check(env, x, splat_sdf_curvature(x, g, sf, n, cur), mk_undefined(env));
}
FN(sdf_seed_positions) { /* (ctx, Float32Array(3) boxMin, Float32Array(3) boxMax, n, seed (integer < 2^53), positions) */
    ARGS(6); splat_ctx *x = arg_external(&c, 0); size_t b0 = 0, b1 = 0; float *mn = arg_hostbuf(&c, 1, &b0), *mx = arg_hostbuf(&c, 2, &b1);
    uint32_t n = (uint32_t)arg_number(&c, 3); double seed = arg_number(&c, 4); void *pos = arg_dptr(&c, 5); BAIL;
    if (b0 < 12 || b1 < 12) { napi_throw_range_error(env, NULL, "sdf_seed_positions: the box corners are three floats each"); return NULL; }
    return check(env, x, splat_sdf_seed_positions(x, mn, mx, n, (uint64_t)seed, pos), mk_undefined(env));
}
FN(sdf_generate) { /* (ctx, program, boxMin | null, boxMax | null, seed, positionsIn | null, n, steps, positionsOut, gradientsOut | null, curvatureOut, propsOut | null) */
    ARGS(12); splat_ctx *x = arg_external(&c, 0); splat_sdf_instr prog[SPLAT_SDF_MAX_INSTR]; uint32_t cnt = 0;
    if (!sdf_program(&c, 1, prog, &cnt)) return NULL;
    napi_valuetype t; napi_typeof(env, c.argv[2], &t);
    float *mn = NULL, *mx = NULL; size_t b0 = 12, b1 = 12;
    if (t != napi_null && t != napi_undefined) { mn = arg_hostbuf(&c, 2, &b0); mx = arg_hostbuf(&c, 3, &b1); }
    double seed = arg_number(&c, 4); void *pin = arg_dptr(&c, 5); uint32_t n = (uint32_t)arg_number(&c, 6), steps = (uint32_t)arg_number(&c, 7);
    void *pout = arg_dptr(&c, 8), *gout = arg_dptr(&c, 9), *cout = arg_dptr(&c, 10), *props = arg_dptr(&c, 11); BAIL;
    if (b0 < 12 || b1 < 12) { napi_throw_range_error(env, NULL, "sdf_generate: the box corners are three floats each"); return NULL; }
    return check(env, x, splat_sdf_generate(x, prog, cnt, mn, mx, (uint64_t)seed, pin, n, steps, pout, gout, cout, props), mk_undefined(env));
}

FN(point_frame) { /* (ctx, binner, Float32Array(22), positions, posStride, gradients, gradStride, scales, scaleStride, n, W, H, out8|null, outF|null, depth|null, ids|null) */
    ARGS(16); splat_ctx *x = arg_external(&c, 0); splat_binner *b = arg_external(&c, 1); size_t ub = 0; float *u = arg_hostbuf(&c, 2, &ub);
    void *pos = arg_dptr(&c, 3); uint32_t ps = (uint32_t)arg_number(&c, 4); void *g = arg_dptr(&c, 5); uint32_t gs = (uint32_t)arg_number(&c, 6);
    void *sc = arg_dptr(&c, 7); uint32_t ss = (uint32_t)arg_number(&c, 8), n = (uint32_t)arg_number(&c, 9);
    uint32_t w = (uint32_t)arg_number(&c, 10), h = (uint32_t)arg_number(&c, 11);
    void *o8 = arg_dptr(&c, 12), *of = arg_dptr(&c, 13), *od = arg_dptr(&c, 14), *oi = arg_dptr(&c, 15); BAIL;
    if (ub < 16 * sizeof(float)) { napi_throw_range_error(env, NULL, "uniform block needs the 16 floats of the view-projection matrix"); return NULL; }
    return check(env, x, splat_point_frame(x, b, u, pos, ps, g, gs, sc, ss, n, w, h, o8, of, od, oi), mk_undefined(env));
}

/* ---- multi-GPU band path (include/splat.h: "multi-GPU band path", "the multi-GPU frame's one exchange") ---- */
FN(project_slice_compact) { /* (ctx, Float32Array(22), posRadius, strideVec4, first, count, records16) */
    ARGS(7); splat_ctx *x = arg_external(&c, 0); size_t ub = 0; float *u = arg_hostbuf(&c, 1, &ub);
    void *pr = arg_dptr(&c, 2); uint32_t st = (uint32_t)arg_number(&c, 3), first = (uint32_t)arg_number(&c, 4), count = (uint32_t)arg_number(&c, 5);
    void *rec = arg_dptr(&c, 6); BAIL;
    if (ub < 22 * sizeof(float)) { napi_throw_range_error(env, NULL, "uniform block needs 22 floats"); return NULL; }
    return check(env, x, splat_project_slice_compact(x, u, pr, st, first, count, rec), mk_undefined(env));
}
FN(band_frame) { /* (ctx, sorter, binner, cfg[8], props, normals|null, records, nRecords, W, H, out8|null, outF|null) */
    ARGS(12); splat_ctx *x = arg_external(&c, 0); splat_sorter *s = arg_external(&c, 1); splat_binner *b = arg_external(&c, 2);
    splat_composite_cfg cfg; fill_cfg(&c, 3, &cfg);
    void *props = arg_dptr(&c, 4), *nrm = arg_dptr(&c, 5), *rec = arg_dptr(&c, 6);
    uint32_t n = (uint32_t)arg_number(&c, 7), w = (uint32_t)arg_number(&c, 8), h = (uint32_t)arg_number(&c, 9);
    void *o8 = arg_dptr(&c, 10), *of = arg_dptr(&c, 11); BAIL;
    int rc = splat_band_frame(x, s, b, &cfg, props, nrm, rec, n, w, h, o8, of, NULL);
    if (AGAIN(rc)) rc = splat_band_frame(x, s, b, &cfg, props, nrm, rec, n, w, h, o8, of, NULL);
    return check(env, x, rc, mk_undefined(env));
}
FN(band_settle) { /* (ctx, sorter, binner) -> pairs of the last band frame (waits for it; throws if it overflowed: render it again) */
    ARGS(3); splat_ctx *x = arg_external(&c, 0); splat_sorter *s = arg_external(&c, 1); splat_binner *b = arg_external(&c, 2); BAIL;
    uint32_t kept = 0; uint64_t pairs = 0;
    int rc = splat_band_settle(x, s, b, &kept, &pairs);
    return check(env, x, rc, rc == SPLAT_OK ? mk_number(env, (double)pairs) : NULL);
}
FN(comm_unique_id) { /* () -> ArrayBuffer(128): rank 0 makes it, every rank passes the same bytes to comm_init */
    (void)info;
    void *data = NULL; napi_value ab;
    if (napi_create_arraybuffer(env, SPLAT_COMM_ID_BYTES, &data, &ab) != napi_ok) return NULL;
    return check(env, NULL, splat_comm_unique_id(data), ab);
}
FN(comm_init) { /* (ctx, rank, world, idBytes) -> comm */
    ARGS(4); splat_ctx *x = arg_external(&c, 0); int rank = (int)arg_number(&c, 1), world = (int)arg_number(&c, 2);
    size_t nb = 0; void *id = arg_hostbuf(&c, 3, &nb); BAIL;
    if (nb < SPLAT_COMM_ID_BYTES) { napi_throw_range_error(env, NULL, "the communicator id is 128 bytes"); return NULL; }
    splat_comm *comm = NULL;
    int rc = splat_comm_init(x, rank, world, id, &comm);
    return check(env, x, rc, rc == SPLAT_OK ? mk_external(env, comm) : NULL);
}
FN(comm_destroy) { ARGS(1); splat_comm_destroy((splat_comm *)arg_external(&c, 0)); return mk_undefined(env); }
FN(allgather_records) { /* (ctx, comm, shard, gathered, bytesPerRank) */
    ARGS(5); splat_ctx *x = arg_external(&c, 0); splat_comm *comm = arg_external(&c, 1);
    void *shard = arg_dptr(&c, 2), *all = arg_dptr(&c, 3); size_t nb = (size_t)arg_number(&c, 4); BAIL;
    return check(env, x, splat_allgather_records(x, comm, shard, all, nb), mk_undefined(env));
}

/* ---- the rest of the ABI: timing detail, composite options, multi-GPU helpers, diagnostics ---- */
static napi_value mk_pair(napi_env env, double a, double b) {
    napi_value arr;
    if (napi_create_array_with_length(env, 2, &arr) != napi_ok) return NULL;
    napi_set_element(env, arr, 0, mk_number(env, a));
    napi_set_element(env, arr, 1, mk_number(env, b));
    return arr;
}
FN(ctx_create_on_stream) { /* (device, hipStream as a number) -> ctx */
    ARGS(2); int dev = (int)arg_number(&c, 0); void *stream = arg_dptr(&c, 1); BAIL;
    splat_ctx *ctx = NULL;
    int rc = splat_ctx_create_on_stream(dev, stream, &ctx);
    return check(env, NULL, rc, rc == SPLAT_OK ? mk_external(env, ctx) : NULL);
}
FN(last_error) { /* (ctx|null) -> string */
    ARGS(1); splat_ctx *x = arg_external(&c, 0); BAIL;
    const char *m = splat_last_error(x);
    napi_value r;
    napi_create_string_utf8(env, m ? m : "", NAPI_AUTO_LENGTH, &r);
    return r;
}
FN(set_timing_stages) { ARGS(2); splat_ctx *x = arg_external(&c, 0); uint32_t m = (uint32_t)arg_number(&c, 1); BAIL; return check(env, x, splat_set_timing_stages(x, m), mk_undefined(env)); }
FN(set_timing_sampling) { ARGS(2); splat_ctx *x = arg_external(&c, 0); uint32_t e = (uint32_t)arg_number(&c, 1); BAIL; return check(env, x, splat_set_timing_sampling(x, e), mk_undefined(env)); }
FN(stage_time_stats) { /* (ctx, stage) -> [samples, totalMs] */
    ARGS(2); splat_ctx *x = arg_external(&c, 0); int st = (int)arg_number(&c, 1); BAIL;
    uint32_t n = 0; double ms = 0;
    int rc = splat_stage_time_stats(x, st, &n, &ms);
    return rc == SPLAT_OK ? mk_pair(env, n, ms) : check(env, x, rc, NULL);
}
FN(timing_consumed) { /* (ctx) -> [staged, consumed] */
    ARGS(1); splat_ctx *x = arg_external(&c, 0); BAIL;
    uint64_t a = 0, b = 0;
    int rc = splat_timing_consumed(x, &a, &b);
    return rc == SPLAT_OK ? mk_pair(env, (double)a, (double)b) : check(env, x, rc, NULL);
}
FN(buf_copy) { /* (ctx, dst, src, bytes) */
    ARGS(4); splat_ctx *x = arg_external(&c, 0); void *d = arg_dptr(&c, 1), *s = arg_dptr(&c, 2); size_t nb = (size_t)arg_number(&c, 3); BAIL;
    return check(env, x, splat_buf_copy(x, d, s, nb), mk_undefined(env));
}
FN(probe_lds_atomic_order) { /* (ctx) -> mismatches */
    ARGS(1); splat_ctx *x = arg_external(&c, 0); BAIL;
    uint64_t m = 0;
    int rc = splat_probe_lds_atomic_order(x, &m);
    return check(env, x, rc, rc == SPLAT_OK ? mk_number(env, (double)m) : NULL);
}
FN(composite_forget_history) { ARGS(1); splat_ctx *x = arg_external(&c, 0); BAIL; return check(env, x, splat_composite_forget_history(x), mk_undefined(env)); }
FN(composite_options) { /* (ctx, kernel, ahead, predict): every call sets all three; -1 (kernel, predict) / 0 (ahead) = the process default (the environment's), as splat.h says */
    ARGS(4); splat_ctx *x = arg_external(&c, 0);
    int k = (int)arg_number(&c, 1), a = (int)arg_number(&c, 2), p = (int)arg_number(&c, 3); BAIL;
    return check(env, x, splat_composite_options(x, k, a, p), mk_undefined(env));
}
FN(bin_dims) { /* (binner) -> [tilesX, tilesY] */
    ARGS(1); splat_binner *b = arg_external(&c, 0); BAIL;
    uint32_t ntx = 0, nty = 0;
    int rc = splat_bin_dims(b, &ntx, &nty);
    return rc == SPLAT_OK ? mk_pair(env, ntx, nty) : check(env, NULL, rc, NULL);
}
FN(bin_tile_size) { ARGS(1); splat_binner *b = arg_external(&c, 0); BAIL; return mk_number(env, splat_bin_tile_size(b)); }
FN(project_slice) { /* (ctx, Float32Array(22), posRadius, strideVec4, first, count, projectedSlice) */
    ARGS(7); splat_ctx *x = arg_external(&c, 0); size_t ub = 0; float *u = arg_hostbuf(&c, 1, &ub);
    void *pr = arg_dptr(&c, 2); uint32_t st = (uint32_t)arg_number(&c, 3), first = (uint32_t)arg_number(&c, 4), count = (uint32_t)arg_number(&c, 5);
    void *out = arg_dptr(&c, 6); BAIL;
    if (ub < 22 * sizeof(float)) { napi_throw_range_error(env, NULL, "uniform block needs 22 floats"); return NULL; }
    return check(env, x, splat_project_slice(x, u, pr, st, first, count, out), mk_undefined(env));
}
FN(project_slice_disc) { /* (ctx, Float32Array(22), posRadius, strideVec4, normals, normalStrideVec4, first, count, records48Slice) */
    ARGS(9); splat_ctx *x = arg_external(&c, 0); size_t ub = 0; float *u = arg_hostbuf(&c, 1, &ub);
    void *pr = arg_dptr(&c, 2); uint32_t st = (uint32_t)arg_number(&c, 3); void *nrm = arg_dptr(&c, 4);
    uint32_t ns = (uint32_t)arg_number(&c, 5), first = (uint32_t)arg_number(&c, 6), count = (uint32_t)arg_number(&c, 7);
    void *out = arg_dptr(&c, 8); BAIL;
    if (ub < 22 * sizeof(float)) { napi_throw_range_error(env, NULL, "uniform block needs 22 floats"); return NULL; }
    return check(env, x, splat_project_slice_disc(x, u, pr, st, nrm, ns, first, count, out), mk_undefined(env));
}
FN(expand_compact) { /* (ctx, records16, n, indexBase, projected) */
    ARGS(5); splat_ctx *x = arg_external(&c, 0); void *rec = arg_dptr(&c, 1);
    uint32_t n = (uint32_t)arg_number(&c, 2), base = (uint32_t)arg_number(&c, 3); void *out = arg_dptr(&c, 4); BAIL;
    return check(env, x, splat_expand_compact(x, rec, n, base, out), mk_undefined(env));
}
FN(band_keys) { /* (ctx, sorter, projected, n, W, H, tile, row0, row1) -> kept */
    ARGS(9); splat_ctx *x = arg_external(&c, 0); splat_sorter *s = arg_external(&c, 1); void *proj = arg_dptr(&c, 2);
    uint32_t n = (uint32_t)arg_number(&c, 3), w = (uint32_t)arg_number(&c, 4), h = (uint32_t)arg_number(&c, 5), t = (uint32_t)arg_number(&c, 6);
    uint32_t r0 = (uint32_t)arg_number(&c, 7), r1 = (uint32_t)arg_number(&c, 8); BAIL;
    uint32_t kept = 0;
    int rc = splat_band_keys(x, s, proj, n, w, h, t, r0, r1, &kept);
    return check(env, x, rc, rc == SPLAT_OK ? mk_number(env, kept) : NULL);
}
FN(band_kept) { /* (ctx, sorter) -> kept */
    ARGS(2); splat_ctx *x = arg_external(&c, 0); splat_sorter *s = arg_external(&c, 1); BAIL;
    uint32_t kept = 0;
    int rc = splat_band_kept(x, s, &kept);
    return check(env, x, rc, rc == SPLAT_OK ? mk_number(env, kept) : NULL);
}
FN(comm_rank) { /* (comm) -> [rank, world] */
    ARGS(1); splat_comm *cm = arg_external(&c, 0); BAIL;
    int r = 0, w = 0;
    int rc = splat_comm_rank(cm, &r, &w);
    return rc == SPLAT_OK ? mk_pair(env, r, w) : check(env, NULL, rc, NULL);
}
FN(comm_count) { /* (comm) -> [ranks RCCL reports, this rank as RCCL reports it] */
    ARGS(1); splat_comm *cm = arg_external(&c, 0); BAIL;
    int n = 0, r = 0;
    int rc = splat_comm_count(cm, &n, &r);
    return rc == SPLAT_OK ? mk_pair(env, n, r) : check(env, NULL, rc, NULL);
}

static napi_value init(napi_env env, napi_value exports) {
#define EXPORT(name) { #name, NULL, name, NULL, NULL, NULL, napi_enumerable, NULL }
    napi_property_descriptor d[] = {
        EXPORT(abi_version), EXPORT(ctx_create), EXPORT(ctx_destroy), EXPORT(sync), EXPORT(rank_status), EXPORT(set_timing), EXPORT(stage_time_ms),
        EXPORT(buf_alloc), EXPORT(buf_free), EXPORT(buf_zero), EXPORT(buf_upload), EXPORT(buf_download), EXPORT(update_props), EXPORT(update_props_planes), EXPORT(props_to_planes), EXPORT(lit_colors),
        EXPORT(project), EXPORT(project_disc), EXPORT(extract_keys), EXPORT(sort_create), EXPORT(sort_destroy), EXPORT(sort_capacity), EXPORT(sort_keys),
        EXPORT(sort_payload), EXPORT(sort_sorted_payload), EXPORT(sort_sorted_keys), EXPORT(sort_run), EXPORT(sort_set_mode),
        EXPORT(scan_u32), EXPORT(bin_create), EXPORT(bin_destroy), EXPORT(bin_run), EXPORT(bin_counts), EXPORT(bin_offsets),
        EXPORT(bin_indices), EXPORT(bin_total), EXPORT(bin_set_frame_order), EXPORT(validate_tile_order), EXPORT(composite), EXPORT(render_frame), EXPORT(render_frame_planes),
        EXPORT(composite_aov), EXPORT(render_frame_aov), EXPORT(render_frame_planes_aov),
        EXPORT(project_slice_compact), EXPORT(band_frame), EXPORT(band_settle), EXPORT(comm_unique_id), EXPORT(comm_init), EXPORT(comm_destroy),
        EXPORT(ctx_create_on_stream), EXPORT(last_error), EXPORT(set_timing_stages), EXPORT(set_timing_sampling), EXPORT(stage_time_stats), EXPORT(timing_consumed),
        EXPORT(buf_copy), EXPORT(probe_lds_atomic_order),
        EXPORT(composite_forget_history), EXPORT(composite_options), EXPORT(bin_dims), EXPORT(bin_tile_size), EXPORT(project_slice),
        EXPORT(project_slice_disc), EXPORT(expand_compact), EXPORT(band_keys), EXPORT(band_kept), EXPORT(comm_rank), EXPORT(comm_count),
        EXPORT(allgather_records), EXPORT(sdf_gradients), EXPORT(sdf_update_positions), EXPORT(sdf_scale_factors), EXPORT(sdf_curvature), EXPORT(sdf_seed_positions), EXPORT(sdf_generate),
        EXPORT(point_frame), EXPORT(project_ellipsoid), EXPORT(sh_colors), EXPORT(render_frame_ellipsoids),
        EXPORT(composite_backward), EXPORT(project_ellipsoid_backward), EXPORT(sh_colors_backward),
        EXPORT(composite_aov_depth), EXPORT(composite_backward_depth), EXPORT(project_ellipsoid_backward_depth),
        EXPORT(composite_backward_det_workspace_bytes), EXPORT(composite_backward_det), EXPORT(composite_contribution),
        EXPORT(project_ellipsoid_backward_camera), EXPORT(sh_colors_backward_camera),
        EXPORT(image_loss_workspace_bytes), EXPORT(image_loss), EXPORT(image_loss_backward),
        EXPORT(camera_rays), EXPORT(depth_normals), EXPORT(depth_normals_backward), EXPORT(normal_consistency),
        EXPORT(normal_consistency_backward),
        EXPORT(tsdf_integrate), EXPORT(tsdf_mesh_workspace_bytes), EXPORT(tsdf_mesh_count), EXPORT(tsdf_mesh_emit),
        EXPORT(adam_step), EXPORT(density_accumulate), EXPORT(densify_plan_workspace_bytes), EXPORT(densify_plan),
        EXPORT(densify_geometry), EXPORT(densify_rows),
        EXPORT(mcmc_sample_workspace_bytes), EXPORT(mcmc_sample), EXPORT(mcmc_apply), EXPORT(mcmc_noise),
        EXPORT(knn_workspace_bytes), EXPORT(knn_mean_sq),
        EXPORT(project_ellipsoid_aa), EXPORT(render_frame_ellipsoids_aa), EXPORT(project_ellipsoid_backward_aa), EXPORT(sampling_rate_max),
        EXPORT(composite_backward_abs), EXPORT(composite_backward_det_abs_workspace_bytes), EXPORT(composite_backward_det_abs),
        EXPORT(density_accumulate_abs), EXPORT(density_accumulate_surfel), EXPORT(densify_plan_surfel), EXPORT(densify_geometry_surfel),
        EXPORT(composite_features), EXPORT(composite_features_backward),
        EXPORT(project_surfel), EXPORT(composite_surfel_depth), EXPORT(composite_surfel_distortion), EXPORT(composite_backward_distortion),
        EXPORT(project_surfel_backward),
    };
    napi_define_properties(env, exports, sizeof d / sizeof d[0], d);
    return exports;
}

NAPI_MODULE(NODE_GYP_MODULE_NAME, init)
