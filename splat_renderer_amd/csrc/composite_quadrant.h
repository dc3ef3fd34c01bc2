// composite_quadrant.h — the one-pixel-per-lane composite: the body k_composite (composite.hip) and k_composite_tile
// (composite_tile.hip) share.
//
// Reference: /root/reference/src/ComputeShaderRenderer.ts:97-198 (evaluateSplat + main, K11),
// dispatched 8x8 with every pixel re-gathering idx/props/normal/projected per list entry
// (:103-115).  CDNA4 design instead:
//   - one 256-thread workgroup per 16x16-pixel WINDOW; wave w owns the 8x8 pixel quadrant w (one pixel per
//     lane, so the 64-wide ballot/all of a wave is exactly "this quadrant").  With 16x16 tiles the window is the tile
//     (k_composite: WINDOWED = false, the tile's edge a compile-time constant); a tile of any other size T is cut into
//     ceil(T/16)^2 windows anchored at its origin, the last window of a row / column clipped to the tile, every window
//     clipped to the screen, each walking its tile's list (k_composite_tile: WINDOWED = true)
//   - the tile's list is consumed in batches of 256 entries: thread t gathers entry t ONCE per window
//     (index, 32 B ProjectedSplat, colour vec4, normal vec4 — the reference's own layouts) and
//     does every per-entry computation there: centre, exp2 scale, lit colour, and for each of the
//     four quadrants the exact 64-bit mask of pixels inside the entry's box (the reference's four
//     float comparisons per pixel per entry become one mask per entry per quadrant; span_mask16, in window-local
//     columns / rows)
//   - each wave reads the 64 masks of a chunk with one LDS read, ballots the non-empty ones and
//     walks only those (s_ff1); an entry whose covered pixels have all saturated is skipped on
//     the scalar unit; the survivors' 32 B of parameters come back as LDS broadcasts
//   - the set of pixels still accumulating is a wave-uniform 64-bit mask: pixels outside the tile or the screen never
//     enter it, a pixel leaves it at alpha >= 0.99 exactly as :187-190 (T_STOP), a wave with none left stops, the workgroup
//     leaves when all four waves have
// A pixel visits its tile's entries in list order whatever the tile size, so the image of every tile size is the 16x16
// kernels' to within the composite's stated tolerance.  Tiles under 16 pixels leave lanes idle (T = 8: three quarters).
//
// Roofline: HBM in the SURVEY §8d model — 68 B per consumed list entry (4 idx + 32 projected +
// 16 colour + 16 normal) + 4 B per pixel written.  The inner loop is VALU/LDS work, so the
// achieved fraction is reported honestly against that model.
//
// Both translation units are compiled with -ffp-contract=on; compared with the oracle within a stated tolerance.
#pragma once
#include "composite.h"

// Where a workgroup works: tile (tx, ty) of the screen, and for WINDOWED = true window (wx, wy) of that tile's wpt x wpt
// windows — pixels [16 wx, 16 wx + 16) x [16 wy, 16 wy + 16) of the tile of T x T pixels, clipped to it.  win_counts: see the
// `consumed` epilogue.  (WINDOWED = false reads tx and ty only.)
struct WindowPlace {
    uint32_t tx, ty;
    uint32_t wx = 0, wy = 0, T = CT, wpt = 1;
    uint2 *win_counts = nullptr;
};

// AOV: also the auxiliary outputs (splat_aov; nearest-on-top only): per staged entry {depth, splat index} beside its
// parameters, per pixel an AovPixel fed with the colour's own weight
// ELL (with DISC): the records are the anisotropic Gaussian's (ellipsoid.h) — the disc footprint with its own exponent scale
template <bool WINDOWED, int MODE, bool EARLY_OUT, bool DISC, bool LIT32, bool AOV, bool ELL>
__device__ __forceinline__ void composite_window(const CompositeParams &p, const WindowPlace &at) {
    // per entry one 32-byte record {centre.x, centre.y, exp2 scale, lit blue | lit red, lit green, -, -}: both
    // halves are read off ONE address register (ds_read_b128 + ds_read_b64 offset:16), and forming an LDS
    // address from the scalar entry index costs a VALU move per register
    // (DISC: {centre.x, centre.y, -q0, -q1 | B00, B10, B01, B11 | lit red, green, blue, -}: B by columns, so that
    // (u,v) numerators are two packed operations on register pairs as they arrive)
    constexpr int PAR = DISC ? 3 : 2;
    __shared__ float4 s_par[CBATCH][PAR];
    __shared__ uint2 s_mask[4][CBATCH];  // per quadrant: which of its 64 pixels the entry's box covers
    __shared__ uint32_t s_wave_done[4];
    __shared__ uint32_t s_wave_consumed[4];
    __shared__ float2 s_aov[AOV ? CBATCH : 1]; // AOV: {depth, splat index} per staged entry
    static_assert(!AOV || MODE == SPLAT_COMPOSITE_FRONT_TO_BACK, "the auxiliary outputs are nearest-on-top only");
    AovPixel aov;

    const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (p.report && blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) tile_report(p.frame_total, p.report, p.report_seq);
    const uint32_t tx = at.tx, ty = at.ty;
    const uint32_t tile_idx = ty * p.ntx + tx; // ComputeShaderRenderer.ts:161-163
    const uint32_t ox = WINDOWED ? tx * at.T + at.wx * CT : tx * CT, oy = WINDOWED ? ty * at.T + at.wy * CT : ty * CT; // the window's origin on the screen
    // (WINDOWED: a window wholly right of or below the screen walks no list: it has no pixel to write)
    const uint32_t count = (!WINDOWED || (ox < p.width && oy < p.height)) ? p.counts[tile_idx] : 0u, off = p.offsets[tile_idx];

    const uint32_t lx = (w & 1) * 8 + (lane & 7), ly = (w >> 1) * 8 + (lane >> 3); // pixel in the window
    // (the 16x16 tile's own spelling: the compiler forms the sum differently from ox + lx, and k_composite keeps its code)
    const uint32_t px = WINDOWED ? ox + lx : tx * CT + (w & 1) * 8 + (lane & 7), py = WINDOWED ? oy + ly : ty * CT + (w >> 1) * 8 + (lane >> 3);
    // in the tile (WINDOWED: the tile's last windows are clipped to it) and on the screen
    const bool pixel_ok = (!WINDOWED || (at.wx * CT + lx < at.T && at.wy * CT + ly < at.T)) && px < p.width && py < p.height;
    const float pxf = (float)px + 0.5f, pyf = (float)py + 0.5f; // :169
    const float win_x0 = (float)ox, win_y0 = (float)oy;
    // (span_mask16's exactness argument holds for any origin: its masks are the reference's box test in window-local columns)
    const float win_cx = win_x0 + 0.5f, win_cy = win_y0 + 0.5f;
    const v2f p_local = {(float)lx + 0.5f, (float)ly + 0.5f}; // pixel centre in the window

    float cr = 0.0f, cg = 0.0f, cb = 0.0f;
    float acc = (MODE == SPLAT_COMPOSITE_REFERENCE_LITERAL) ? 0.0f : 1.0f; // alpha (literal) or transmittance T
    // wave-uniform mask of the pixels still accumulating; a pixel leaves it when its alpha reaches
    // 0.99 (:187-190) and pixels outside the image never enter it
    unsigned long long live = uniform64(__ballot(pixel_ok));
    if (tid < 4) s_wave_done[tid] = 0;

    uint32_t staged = 0;
    // list entries this wave needed: the position after the entry at which its last pixel saturated, or the whole
    // list if some pixel never did (SURVEY §8d's P_used per tile = the largest over its windows' waves; = count with early-out off)
    uint32_t needed = 0;

    // ---- list-entry fetch, split from its use (issue early / write LDS late).  Almost every tile
    // saturates inside its first batch, but tiles on a silhouette keep some pixel open and walk
    // their whole list (thousands of entries): from their second batch on, the NEXT batch's gathers
    // are issued before the current batch is consumed, so the ~3 us dependent-load chain (index, then
    // record / colour / normal) overlaps the arithmetic instead of preceding it.
    uint32_t f_idx = 0xffffffffu;              // splat index of the entry this thread stages
    float4 f_b = make_float4(0, 0, 0, 0), f_c = f_b, f_n = f_b, f_b2 = f_b;
    float f_r = 0.0f;
    float2 f_zi = make_float2(0.0f, 0.0f);     // AOV: {depth, index} of that entry, fetched with it
    bool f_ready = false;                      // f_* already hold this thread's entry of the batch about to be staged
    uint32_t n_idx = 0xffffffffu;              // index of this thread's entry one batch further on (the gathers depend on it)
    bool n_idx_valid = false;

    for (uint32_t base = 0; base < count; base += CBATCH) {
        __syncthreads(); // previous batch fully consumed (and s_wave_done visible)
        if (EARLY_OUT) {
            // (readfirstlane: an LDS value is "divergent" to the compiler, which would then treat
            // this whole loop, and every mask carried through it, as per-lane)
            if (__builtin_amdgcn_readfirstlane((int)(s_wave_done[0] & s_wave_done[1] & s_wave_done[2] & s_wave_done[3]))) break;
        }
        // ---- stage: one entry per thread, everything per-entry is computed here, once per window ----
        {
            const uint32_t e = base + tid;
            float4 geo = make_float4(0.0f, 0.0f, 0.0f, 0.0f), geo2 = geo;
            float2 col = make_float2(0.0f, 0.0f);
            float col_b = 0.0f, col_o = 0.0f;
            uint32_t xm = 0, ym = 0;
            if (!f_ready) { // the first three batches of a tile: fetch now
                f_idx = (tid < CBATCH && e < count) ? p.indices[off + e] : 0xffffffffu;
                if (f_idx != 0xffffffffu) fetch_entry<MODE, EARLY_OUT, DISC, LIT32, ELL>(p, f_idx, f_b, f_b2, f_c, f_n, f_r);
                if constexpr (AOV) f_zi = aov_entry(p, f_idx);
            }
            if (DISC && f_idx != 0xffffffffu) {
                const DiscRecord rec = {f_b, f_b2};
                float4 bnd;
                if (disc_bounds(rec, bnd)) { // (a culled splat's record is all zeros and is in no list anyway)
                    const float4 c = (p.prelit || p.disc_lit) ? f_c : lit_color(f_c, f_n);
                    col = make_float2(c.x, c.y);
                    col_b = c.z;
                    col_o = c.w;
                    geo = make_float4(f_b.x, f_b.y, -f_b2.z, -f_b2.w);
                    geo2 = make_float4(f_b.z, f_b2.x, f_b.w, f_b2.y);
                    xm = span_mask16(bnd.x, bnd.z, win_cx);
                    ym = span_mask16(bnd.y, bnd.w, win_cy);
                }
            }
            if (!DISC && f_idx != 0xffffffffu) {
                const float4 b = f_b;
                const float r = f_r;
                if (!(r < 0.5f)) { // :127-129 "too small"
                    const float4 c = (LIT32 || p.prelit) ? f_c : lit_color(f_c, f_n);
                    col = make_float2(c.x, c.y);
                    // gaussian = exp(-0.5 nd^2 / 0.25), nd = dist / r  ->  exp2(-((dx k)^2 + (dy k)^2)), k = sqrt(2 log2 e) / r,
                    // evaluated per pixel as (p k - c k)^2 in WINDOW-LOCAL coordinates (|p|, |c| of the order of the window, so the
                    // difference loses nothing that matters: < 1e-5 relative in the Gaussian for the smallest splat the
                    // reference draws): one packed multiply-add, one packed square and an add per (entry, quadrant) instead of
                    // two subtractions, two multiplies and a scale — the kernel is bound by vector-ALU issue slots
                    const float k = 1.6986436005760381f / r;                                     // sqrt(2.885390081777927)
                    const float cx = (b.x + b.z) * 0.5f - win_x0, cy = (b.y + b.w) * 0.5f - win_y0; // :124, then exact
                    geo = make_float4(cx * k, cy * k, k, c.z);
                    xm = span_mask16(b.x, b.z, win_cx);
                    ym = span_mask16(b.y, b.w, win_cy);
                }
            }
            if (tid < CBATCH) {
                s_par[tid][0] = geo;
                if constexpr (DISC) {
                    s_par[tid][1] = geo2;
                    s_par[tid][2] = make_float4(col.x, col.y, col_b, ELL ? col_o : 0.0f);
                } else {
                    s_par[tid][1] = make_float4(col.x, col.y, 0.0f, 0.0f);
                }
                s_mask[0][tid] = quadrant_mask(xm & 0xffu, ym & 0xffu);
                s_mask[1][tid] = quadrant_mask(xm >> 8, ym & 0xffu);
                s_mask[2][tid] = quadrant_mask(xm & 0xffu, ym >> 8);
                s_mask[3][tid] = quadrant_mask(xm >> 8, ym >> 8);
                if constexpr (AOV) s_aov[tid] = f_zi;
            }
            // issue the fetches for later batches; nothing below waits for them until the next stage
            f_ready = false;
            if (base >= CBATCH) { // a tile that needed a second batch usually needs more
                if (n_idx_valid) { // index of batch k+1 arrived a batch ago: its gathers go out now
                    f_idx = n_idx;
                    if (f_idx != 0xffffffffu) fetch_entry<MODE, EARLY_OUT, DISC, LIT32, ELL>(p, f_idx, f_b, f_b2, f_c, f_n, f_r);
                    if constexpr (AOV) f_zi = aov_entry(p, f_idx);
                    f_ready = true;
                }
                const uint32_t e2 = e + 2 * CBATCH; // batch k+2
                n_idx = (tid < CBATCH && e2 < count) ? p.indices[off + e2] : 0xffffffffu;
                n_idx_valid = true;
            }
        }
        staged = (count - base < CBATCH) ? count : base + CBATCH;
        __syncthreads();
        if (uniform64(live) == 0) { // nothing left to accumulate (or a quadrant wholly outside the image)
            if (EARLY_OUT && lane == 0) s_wave_done[w] = 1;
            continue;
        }
        // ---- consume: 4 chunks of 64 entries; lane j looks at entry c0+j's mask for this quadrant ---
        const uint32_t batch_n = (count - base < CBATCH) ? (count - base) : CBATCH;
        needed = base + batch_n; // unless the wave saturates inside this batch (below)
        for (uint32_t c0 = 0; c0 < batch_n && uniform64(live) != 0; c0 += 64) {
            const uint2 mm = s_mask[w][c0 + lane];
            // entries of this chunk that cover at least one pixel still accumulating
            const unsigned long long lv0 = uniform64(live);
            unsigned long long hits = uniform64(__ballot(((mm.x & (uint32_t)lv0) | (mm.y & (uint32_t)(lv0 >> 32))) != 0u));
            // two entries per trip: both parameter reads are in flight together, both Gaussians are
            // independent work, and the loop/branch overhead is paid once per pair; the second
            // entry's coverage is re-masked with the pixels the first one has just saturated, so the
            // per-pixel stop is exactly sequential
            bool saturated = false; // (one loop exit: the accumulators then stay in the registers they live in)
            while (hits && !saturated) {
                const uint32_t j0 = (uint32_t)__builtin_ctzll(hits);
                hits &= hits - 1;
                const bool two = hits != 0;
                const uint32_t j1 = two ? (uint32_t)__builtin_ctzll(hits) : j0;
                hits &= hits - 1; // (0 & anything stays 0)
                // (readlane returns int: go through uint32_t or the low word sign-extends into the high one)
                const unsigned long long cover0 = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)mm.y, (int)j0) << 32) |
                                                  (unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)mm.x, (int)j0);
                unsigned long long cover1 = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)mm.y, (int)j1) << 32) |
                                            (unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)mm.x, (int)j1);
                if (!two) cover1 = 0;
                const float4 G0 = s_par[c0 + j0][0], G1 = s_par[c0 + j1][0]; // wave-uniform addresses: LDS broadcasts
                float2 C0, C1;
                float B0, B1, g0, g1; // blue, Gaussian
                if constexpr (DISC) {
                    const float4 M0 = s_par[c0 + j0][1], M1 = s_par[c0 + j1][1];
                    const float4 L0 = s_par[c0 + j0][2], L1 = s_par[c0 + j1][2];
                    C0 = make_float2(L0.x, L0.y); B0 = L0.z;
                    C1 = make_float2(L1.x, L1.y); B1 = L1.z;
                    const v2f pc = {pxf, pyf};
                    const v2f e0 = pc - (v2f){G0.x, G0.y}, e1 = pc - (v2f){G1.x, G1.y};
                    const float rd0 = __builtin_amdgcn_rcpf(__builtin_fmaf(G0.z, e0.x, __builtin_fmaf(G0.w, e0.y, 1.0f))); // 1 / (1 - q.d)
                    const float rd1 = __builtin_amdgcn_rcpf(__builtin_fmaf(G1.z, e1.x, __builtin_fmaf(G1.w, e1.y, 1.0f)));
                    const v2f uv0 = ((v2f){M0.x, M0.y} * e0.x + (v2f){M0.z, M0.w} * e0.y) * rd0; // B*d / (1 - q.d)
                    const v2f uv1 = ((v2f){M1.x, M1.y} * e1.x + (v2f){M1.z, M1.w} * e1.y) * rd1;
                    const float d0 = uv0.x * uv0.x + uv0.y * uv0.y, d1 = uv1.x * uv1.x + uv1.y * uv1.y; // :126
                    g0 = (d0 <= 1.0f) ? __builtin_amdgcn_exp2f(d0 * FootprintExp2<ELL>::scale) : 0.0f; // :128-133 (NaN: outside)
                    g1 = (d1 <= 1.0f) ? __builtin_amdgcn_exp2f(d1 * FootprintExp2<ELL>::scale) : 0.0f;
                    if constexpr (ELL) { // alpha = opacity g (the ellipsoid's opacity rides in the colour's fourth word)
                        g0 *= L0.w;
                        g1 *= L1.w;
                    }
                } else {
                    C0 = *reinterpret_cast<const float2 *>(&s_par[c0 + j0][1]);
                    C1 = *reinterpret_cast<const float2 *>(&s_par[c0 + j1][1]);
                    B0 = G0.w;
                    B1 = G1.w;
                    const v2f t0 = p_local * (v2f){G0.z, G0.z} - (v2f){G0.x, G0.y}, t1 = p_local * (v2f){G1.z, G1.z} - (v2f){G1.x, G1.y};
                    const v2f q0 = t0 * t0, q1 = t1 * t1;
                    g0 = __builtin_amdgcn_exp2f(-(q0.x + q0.y));
                    g1 = __builtin_amdgcn_exp2f(-(q1.x + q1.y));
                }
                unsigned long long lv = uniform64(live); // pinned at the use: see uniform64()
                g0 = __builtin_amdgcn_inverse_ballot_w64(cover0 & lv) ? g0 : 0.0f;
                if (MODE == SPLAT_COMPOSITE_REFERENCE_LITERAL) { // :183-185 as written
                    const float om = 1.0f - g0;
                    cr = cr * om + C0.x * g0;
                    cg = cg * om + C0.y * g0;
                    cb = cb * om + B0 * g0;
                    acc = acc * om + g0;
                    if (EARLY_OUT) lv &= ~__ballot(acc >= 0.99f); // :187-190
                } else { // SURVEY §8a contract 3: nearest on top
                    const float wgt = acc * g0;
                    cr += C0.x * wgt;
                    cg += C0.y * wgt;
                    cb += B0 * wgt;
                    acc -= wgt; // T * (1 - g), with the product already in hand
                    if constexpr (AOV) aov.add(wgt, s_aov[c0 + j0]);
                    if (EARLY_OUT) lv &= ~__ballot(acc <= T_STOP);
                }
                lv = uniform64(lv);
                const bool first_saturated = lv == 0; // (scalar; only read on the way out)
                g1 = __builtin_amdgcn_inverse_ballot_w64(cover1 & lv) ? g1 : 0.0f;
                if (MODE == SPLAT_COMPOSITE_REFERENCE_LITERAL) {
                    const float om = 1.0f - g1;
                    cr = cr * om + C1.x * g1;
                    cg = cg * om + C1.y * g1;
                    cb = cb * om + B1 * g1;
                    acc = acc * om + g1;
                    if (EARLY_OUT) lv &= ~__ballot(acc >= 0.99f);
                } else {
                    const float wgt = acc * g1;
                    cr += C1.x * wgt;
                    cg += C1.y * wgt;
                    cb += B1 * wgt;
                    acc -= wgt;
                    if constexpr (AOV) aov.add(wgt, s_aov[c0 + j1]);
                    if (EARLY_OUT) lv &= ~__ballot(acc <= T_STOP);
                }
                live = lv;
                if (EARLY_OUT && uniform64(live) == 0) {
                    needed = base + c0 + (first_saturated ? j0 : j1) + 1;
                    saturated = true;
                }
            }
        }
        if (EARLY_OUT && uniform64(live) == 0 && lane == 0) s_wave_done[w] = 1;
    }

    // per tile {entries staged, entries consumed}: the largest over the tile's windows (each walks the same list).  A tile of one
    // window adds them to the counters itself (per tile, no atomics: 8160 workgroups adding to ONE counter cost the kernel
    // 30 us at C1 and 80 us at C3 — the measurement was slowing down what it measured); otherwise each window leaves its pair
    // in win_counts and k_window_counts adds the tile's largest after the launch (device-scope atomics with fences between
    // a tile's windows made the counting launch 4-6x slower at C2)
    if (p.consumed) { // (uniform branch; timed / diagnostic runs only)
        if (lane == 0) s_wave_consumed[w] = needed;
        __syncthreads();
        if (tid == 0) {
            const uint32_t used = max(max(s_wave_consumed[0], s_wave_consumed[1]), max(s_wave_consumed[2], s_wave_consumed[3]));
            if (!WINDOWED || at.wpt == 1) {
                if (staged) {
                    p.consumed[(size_t)tile_idx * 2] += (unsigned long long)staged;
                    p.consumed[(size_t)tile_idx * 2 + 1] += (unsigned long long)used;
                }
            } else {
                at.win_counts[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = make_uint2(staged, used);
            }
        }
    }

    if (pixel_ok) {
        const float rem = (MODE == SPLAT_COMPOSITE_REFERENCE_LITERAL) ? (1.0f - acc) : acc;
        const float fr = cr + 0.05f * rem, fg = cg + 0.05f * rem, fb = cb + 0.1f * rem; // :193-195
        const size_t o = (size_t)py * p.width + px;
        if (p.out_rgba8) p.out_rgba8[o] = unorm8(fr) | (unorm8(fg) << 8) | (unorm8(fb) << 16) | (255u << 24);
        if (p.out_rgba32f) p.out_rgba32f[o] = make_float4(fr, fg, fb, 1.0f);
        if constexpr (AOV) aov.store(p, o, acc);
    }
}
