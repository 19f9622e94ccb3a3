// zs_slide_body.h — the per-bin workgroup body of the block-initialised sliding DFT: a statement list,
// included inside a kernel's function body (see zs_body.h; no include guard on purpose).  In scope:
// a (ZsArgs), zsm (dynamic LDS), cx (a context), NB, BPL, DEFER, OUT.
    constexpr int LPC = 64 / BPL;                                      // lanes per chunk row
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int W = a.W, C = a.C, N = a.N, NQ = N / C;
    const int STG = zs_stg(C, BPL);                                    // per-wave staging per branch
    int64_t c0, c1;
    cx.chunks(a, BPL, W, c0, c1);
    const int nblk = (int)(c1 - c0) + NQ - 1;
    double2* beta = zsm;                                               // [nblk][NB][64]
    double2* stg = zsm + (size_t)(BPL * W + NQ - 1) * NB * 64 + (size_t)w * NB * STG;   // per wave [NB][STG]

    // ---- phase 1: block DFTs (lane = bin slot) ----
    zs_blocks<NB>(a, cx, beta, stg, STG, cx.row0(0), c0, nblk, lane, w);
    __syncthreads();

    // ---- phase 2: BPL chunks per wave, BPL bins per lane ----
    const int row = lane / LPC, sl = lane % LPC;
    const int64_t c = c0 + BPL * (int64_t)w + row;                     // this row's chunk
    const bool idle = c0 + BPL * (int64_t)w >= c1;                     // no chunk for the whole wave
    if (!DEFER && idle) return;                                        // (no barrier follows)
    const bool live = c < c1;
    const int cl = live ? (int)(c - c0) : 0;                           // local block of the window start
    double2 cq[BPL], tq[BPL], X[BPL][NB];
#pragma unroll
    for (int q = 0; q < BPL; ++q) {
        const int slot = sl + LPC * q;
        const bool valid = slot < a.nbins;
        const int k = valid ? a.kb[slot] : 0;
        const double2 wk = twid(k, N);
        cq[q] = valid ? make_double2(wk.x, -wk.y) : make_double2(0.0, 0.0);   // w^{-k}; 0 holds a slot at 0
        tq[q] = valid ? make_double2(a.tr[slot], a.ti[slot]) : make_double2(0.0, 0.0);
        const double2 step = twid(((int64_t)k * C) % N, N);            // w^{kC}
        double2 t = make_double2(1.0, 0.0);
#pragma unroll
        for (int r = 0; r < NB; ++r) X[q][r] = make_double2(0.0, 0.0);
        for (int p = 0; p < (idle ? 0 : NQ); ++p) {
#pragma unroll
            for (int r = 0; r < NB; ++r) X[q][r] = cfma(t, beta[((cl + p) * NB + r) * 64 + slot], X[q][r]);
            t = cmul(t, step);
        }
#pragma unroll
        for (int r = 0; r < NB; ++r)
            if (!valid) X[q][r] = make_double2(0.0, 0.0);
    }
    double2* dbuf = stg;                                               // [NB][BPL rows][ZS_G]
    const int64_t o0 = c * (int64_t)C;
    OUT* out = cx.out(a);
        if constexpr (DEFER) {
        // the block DFTs are dead once every wave has its initial windows: their region holds
        // the per-wave partials [ZS_RG steps][cr, ci, e][64 lanes] (6.1 KiB <= 8·NB·BPL/8 KiB per wave)
        __syncthreads();
        if (idle) return;
        double* part = reinterpret_cast<double*>(zsm) + (size_t)w * (ZS_RG * ZS_PS);
        constexpr int KD = ZS_G / ZS_RG;                               // partial rounds per group
        for (int og = 0; og < C; og += ZS_G) {
            zs_stage_d<NB, LPC, BPL>(a, cx, dbuf, o0, og, live, row, sl);
            wave_sync();
#pragma unroll 1
            for (int v = 0; v < KD; ++v) {
#pragma unroll OFS_ZS_DUNROLL
                for (int uu = 0; uu < ZS_RG; ++uu) {
                    const int u = v * ZS_RG + uu;
                    double cr = 0.0, ci = 0.0, e = 0.0;
#pragma unroll
                    for (int q = 0; q < BPL; ++q) {
                        double sr = X[q][0].x, si = X[q][0].y;
#pragma unroll
                        for (int r = 1; r < NB; ++r) { sr += X[q][r].x; si += X[q][r].y; }
                        cr = fma(tq[q].x, sr, fma(tq[q].y, si, cr));   // conj(t) · Σ_br X
                        ci = fma(tq[q].x, si, fma(-tq[q].y, sr, ci));
#pragma unroll
                        for (int r = 0; r < NB; ++r) e = fma(X[q][r].x, X[q][r].x, fma(X[q][r].y, X[q][r].y, e));
                    }
                    part[uu * ZS_PS + lane] = cr;
                    part[uu * ZS_PS + 64 + lane] = ci;
                    part[uu * ZS_PS + 128 + lane] = e;
#pragma unroll
                    for (int r = 0; r < NB; ++r) {
                        const double2 d = dbuf[(r * BPL + row) * ZS_G + u];
#pragma unroll
                        for (int q = 0; q < BPL; ++q)
                            X[q][r] = cmul(make_double2(X[q][r].x + d.x, X[q][r].y + d.y), cq[q]);
                    }
                }
                wave_sync();
                if (sl < ZS_RG) {                                      // lane (row, j): step v·RG + j
                    const double* p = part + sl * ZS_PS + row * LPC;
                    double sr = 0.0, si = 0.0, se = 0.0;
#pragma unroll
                    for (int l = 0; l < LPC; l += 2) {
                        const double2 pr = *reinterpret_cast<const double2*>(p + l);
                        const double2 pi = *reinterpret_cast<const double2*>(p + 64 + l);
                        const double2 pe = *reinterpret_cast<const double2*>(p + 128 + l);
                        sr += pr.x + pr.y;
                        si += pi.x + pi.y;
                        se += pe.x + pe.y;
                    }
                    const int64_t s = o0 + og + v * ZS_RG + sl;
                    if (live && cx.stored(a, s)) {
                        const double den = a.t_energy * se;
                        out[s] = (OUT)(fma(sr, sr, si * si) / (den > 1e-12 ? den : 1e-12));
                    }
                }
                wave_sync();                                           // partials rewritten next round
            }
        }
        return;
    }
    constexpr int KEEP = ZS_G / LPC;                                   // results kept per lane per group
    for (int og = 0; og < C; og += ZS_G) {
#pragma unroll
        for (int j = 0; j < KEEP; ++j) {
            const int64_t s = o0 + og + sl + LPC * j;                  // offsets of this lane's loads
            const int64_t i0 = a.cp + s;
#pragma unroll
            for (int r = 0; r < NB; ++r) {
                double2 d = make_double2(0.0, 0.0);
                if (live && s < cx.end(a) && i0 + N < cx.len(a)) {
                    double2 u, v;
                    cx.ld2(a, r, i0, N, u, v);
                    d = make_double2(u.x - v.x, u.y - v.y);
                }
                dbuf[(r * BPL + row) * ZS_G + sl + LPC * j] = d;
            }
        }
        wave_sync();
        double keep_n[KEEP], keep_e[KEEP];
#pragma unroll
        for (int j = 0; j < KEEP; ++j) { keep_n[j] = 0.0; keep_e[j] = 0.0; }
#pragma unroll OFS_ZS_UNROLL
        for (int u = 0; u < ZS_G; ++u) {
            double cr = 0.0, ci = 0.0, e = 0.0;
#pragma unroll
            for (int q = 0; q < BPL; ++q) {
                double sr = X[q][0].x, si = X[q][0].y;
#pragma unroll
                for (int r = 1; r < NB; ++r) { sr += X[q][r].x; si += X[q][r].y; }
                cr = fma(tq[q].x, sr, fma(tq[q].y, si, cr));           // conj(t) · Σ_br X
                ci = fma(tq[q].x, si, fma(-tq[q].y, sr, ci));
#pragma unroll
                for (int r = 0; r < NB; ++r) e = fma(X[q][r].x, X[q][r].x, fma(X[q][r].y, X[q][r].y, e));
            }
            cr = row_sum<LPC>(cr);
            ci = row_sum<LPC>(ci);
            e = row_sum<LPC>(e);
            const double n2 = fma(cr, cr, ci * ci);
#pragma unroll
            for (int j = 0; j < KEEP; ++j)
                if (u == sl + LPC * j) { keep_n[j] = n2; keep_e[j] = e; }
#pragma unroll
            for (int r = 0; r < NB; ++r) {
                const double2 d = dbuf[(r * BPL + row) * ZS_G + u];
#pragma unroll
                for (int q = 0; q < BPL; ++q)
                    X[q][r] = cmul(make_double2(X[q][r].x + d.x, X[q][r].y + d.y), cq[q]);
            }
        }
        wave_sync();                                                   // dbuf rewritten next group
#pragma unroll
        for (int j = 0; j < KEEP; ++j) {
            const int64_t s = o0 + og + sl + LPC * j;
            if (live && cx.stored(a, s)) {
                const double den = a.t_energy * keep_e[j];
                out[s] = (OUT)(keep_n[j] / (den > 1e-12 ? den : 1e-12));
            }
        }
    }
