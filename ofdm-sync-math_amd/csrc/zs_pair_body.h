// zs_pair_body.h — the mirror-pair workgroup body of the block-initialised sliding DFT: a statement
// list, included inside a kernel's function body (see zs_body.h; no include guard on purpose).  In
// scope: a (ZsArgs), zsm (dynamic LDS), cx (a context), NB, PPL, DEFER, OUT.
    constexpr int LPC = 32 / PPL;                                      // lanes per chunk row
    constexpr int ROWS = 64 / LPC;                                     // chunks per wave
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int W = a.W, C = a.C, N = a.N, NQ = N / C;
    int64_t c0, c1;
    cx.chunks(a, ROWS, W, c0, c1);
    const int nblk = (int)(c1 - c0) + NQ - 1;
    // Blocks of ONE branch at a time (NBB = 1 row of 64 slots per block): the branch's initial windows
    // are built from them before the next branch's blocks overwrite the region, so the workgroup's LDS
    // holds one branch's blocks (two branches: half the LDS, twice the resident workgroups)
    constexpr int NBB = 1;
    double2* beta = zsm;                                               // [nblk][NBB][64]
    double2* stg = zsm + (size_t)(ROWS * W + NQ - 1) * NBB * 64 + (size_t)w * zs_pair_stgw(C, ROWS, NB);

    const int row = lane / LPC, sl = lane % LPC;
    const int64_t c = c0 + ROWS * (int64_t)w + row;
    const bool idle = c0 + ROWS * (int64_t)w >= c1;
    const bool live = c < c1;
    const int cl = live ? (int)(c - c0) : 0;
    double2 g[PPL][NB], h[PPL][NB];
    double epp = 0.0;                                                  // Σ |h|² (last step's Σ |g|²)
#pragma unroll
    for (int rb = 0; rb < NB; ++rb) {
        if (rb > 0) __syncthreads();                                   // the previous branch's blocks are read
        if (a.gblk)
            zs_blocks_pair<NBB>(a, cx, beta, stg, zs_stg(C, ROWS), cx.row0(rb), c0, nblk, lane, w);
        else
            zs_blocks<NBB>(a, cx, beta, stg, zs_stg(C, ROWS), cx.row0(rb), c0, nblk, lane, w);
        __syncthreads();
        // branch rb's initial windows: X_s[±k] = Σ_{q<N/C} w^{±kqC} β_{±k}(c + q)
#pragma unroll
        for (int q = 0; q < PPL; ++q) {
            const int p = sl + LPC * q;
            const bool valid = p < a.npairs && !idle;
            const int k = valid ? a.pk[p] : 1, sp = valid ? a.ps[p] : 0, sn = valid ? a.pn[p] : 0;
            const double2 w1 = twid(k, N);
            const double inv2s = -0.5 / w1.y;                          // 1 / (2 sin θ)
            const double2 step = twid(((int64_t)k * C) % N, N);        // w^{kC}
            double2 t = make_double2(1.0, 0.0), xp = make_double2(0.0, 0.0), xn = make_double2(0.0, 0.0);
            for (int pq = 0; pq < (valid ? NQ : 0); ++pq) {
                xp = cfma(t, beta[(cl + pq) * NBB * 64 + sp], xp);
                xn = cfma(make_double2(t.x, -t.y), beta[(cl + pq) * NBB * 64 + sn], xn);
                t = cmul(t, step);
            }
            const double2 yp = cmul(w1, xp), yn = cmul(make_double2(w1.x, -w1.y), xn);
            const double2 hh = make_double2((yp.y - yn.y) * inv2s, -(yp.x - yn.x) * inv2s);   // -i(y+ - y-)/(2 sin θ)
            const double2 gg = cfma(w1, hh, yp);
            h[q][rb] = valid ? hh : make_double2(0.0, 0.0);
            g[q][rb] = valid ? gg : make_double2(0.0, 0.0);
            epp = fma(h[q][rb].x, h[q][rb].x, fma(h[q][rb].y, h[q][rb].y, epp));
        }
    }
    if (!DEFER && idle) return;                                        // (no barrier follows)
    double c2[PPL], dm[PPL];
    double2 A[PPL], Bc[PPL];
#pragma unroll
    for (int q = 0; q < PPL; ++q) {
        const int p = sl + LPC * q;
        const bool valid = p < a.npairs && !idle;
        const int k = valid ? a.pk[p] : 1, sp = valid ? a.ps[p] : 0, sn = valid ? a.pn[p] : 0;
        const double2 w1 = twid(k, N);                                 // w^k = e^{-iθ}
        const double2 tp = make_double2(a.tr[sp], -a.ti[sp]), tn = make_double2(a.tr[sn], -a.ti[sn]);  // conj(t±)
        const double2 ap = cmul(tp, make_double2(w1.x, -w1.y)), an = cmul(tn, w1);
        A[q] = valid ? make_double2(ap.x + an.x, ap.y + an.y) : make_double2(0.0, 0.0);
        Bc[q] = valid ? make_double2(-(tp.x + tn.x), -(tp.y + tn.y)) : make_double2(0.0, 0.0);
        c2[q] = valid ? 2.0 * w1.x : 0.0;
        dm[q] = valid ? 1.0 : 0.0;
    }
    double2* dbuf = stg;                                               // [NB][ROWS][ZS_G]
    const int64_t o0 = c * (int64_t)C;
    OUT* out = cx.out(a);
        // one offset: in-lane partials (numerator, energy) of the lane's pairs from (cur, prv) = (g, h)
    // or (h, g); the update writes the new g over prv, so two consecutive steps swap the roles of the
    // two register sets and no state is copied
    // sg[q] (two branches): the branch sum of the set that is `prv` in the coming step - a step's h
    // sums are the previous step's g sums, so each step forms only the g sums
    double2 sg[NB > 1 ? PPL : 1];
#pragma unroll
    for (int q = 0; q < (NB > 1 ? PPL : 0); ++q) {
        double sx = h[q][0].x, sy = h[q][0].y;
#pragma unroll
        for (int r = 1; r < NB; ++r) { sx += h[q][r].x; sy += h[q][r].y; }
        sg[q] = make_double2(sx, sy);
    }
    // e: HALF the energy (|g|² + |h|² - c2·Re(g h*) summed); the factor 2 sits in the denominator
    auto step_terms = [&](const double2 (&cur)[PPL][NB], const double2 (&prv)[PPL][NB], double& cr, double& ci,
                          double& e) {
        double ep = 0.0, ed = 0.0;
        cr = 0.0; ci = 0.0;
#pragma unroll
        for (int q = 0; q < PPL; ++q) {
            double gr = cur[q][0].x, gim = cur[q][0].y;
#pragma unroll
            for (int r = 1; r < NB; ++r) { gr += cur[q][r].x; gim += cur[q][r].y; }
            double hr = prv[q][0].x, him = prv[q][0].y;
            if constexpr (NB > 1) {
                hr = sg[q].x; him = sg[q].y;
                sg[q] = make_double2(gr, gim);
            }
            cr = fma(A[q].x, gr, fma(-A[q].y, gim, fma(Bc[q].x, hr, fma(-Bc[q].y, him, cr))));
            ci = fma(A[q].x, gim, fma(A[q].y, gr, fma(Bc[q].x, him, fma(Bc[q].y, hr, ci))));
            double t = cur[q][0].y * prv[q][0].y;                      // Σ_br Re(g h*)
            t = fma(cur[q][0].x, prv[q][0].x, t);
#pragma unroll
            for (int r = 1; r < NB; ++r) t = fma(cur[q][r].x, prv[q][r].x, fma(cur[q][r].y, prv[q][r].y, t));
#pragma unroll
            for (int r = 0; r < NB; ++r) ep = fma(cur[q][r].x, cur[q][r].x, fma(cur[q][r].y, cur[q][r].y, ep));
            ed = fma(c2[q], t, ed);
        }
        e = (ep + epp) - ed;
        epp = ep;
    };
    const double te2 = 2.0 * a.t_energy;                               // template energy x the energy's 2
    auto advance = [&](const double2 (&cur)[PPL][NB], double2 (&prv)[PPL][NB], int u) {
#pragma unroll
        for (int r = 0; r < NB; ++r) {
            const double2 d = dbuf[(r * ROWS + row) * ZS_G + u];
#pragma unroll
            for (int q = 0; q < PPL; ++q) {
                const double2 tq = make_double2(fma(dm[q], d.x, -prv[q][r].x), fma(dm[q], d.y, -prv[q][r].y));
                prv[q][r] = make_double2(fma(c2[q], cur[q][r].x, tq.x), fma(c2[q], cur[q][r].y, tq.y));
            }
        }
    };
    if constexpr (DEFER) {
        __syncthreads();                                               // blocks dead: partials take their place
        if (idle) return;
        double* part = reinterpret_cast<double*>(zsm) + (size_t)w * (ZS_RG * ZS_PS);
        for (int og = 0; og < C; og += ZS_G) {
            zs_stage_d<NB, LPC, ROWS>(a, cx, dbuf, o0, og, live, row, sl);
            wave_sync();
#pragma unroll 1
            for (int v = 0; v < ZS_G / ZS_RG; ++v) {
#pragma unroll 1
                for (int uu = 0; uu < ZS_RG; uu += 2) {
                    double cr, ci, e;
                    step_terms(g, h, cr, ci, e);
                    part[uu * ZS_PS + lane] = cr;
                    part[uu * ZS_PS + 64 + lane] = ci;
                    part[uu * ZS_PS + 128 + lane] = e;
                    advance(g, h, v * ZS_RG + uu);                     // h <- new state
                    step_terms(h, g, cr, ci, e);
                    part[(uu + 1) * ZS_PS + lane] = cr;
                    part[(uu + 1) * ZS_PS + 64 + lane] = ci;
                    part[(uu + 1) * ZS_PS + 128 + lane] = e;
                    advance(h, g, v * ZS_RG + uu + 1);                 // g <- new state
                }
                wave_sync();
                if (sl < ZS_RG) {                                      // lane (row, j): step v·RG + j
                    const double* pp = part + sl * ZS_PS + row * LPC;
                    double sr = 0.0, si = 0.0, se = 0.0;
#pragma unroll
                    for (int l = 0; l < LPC; l += 2) {
                        const double2 pr = *reinterpret_cast<const double2*>(pp + l);
                        const double2 pi = *reinterpret_cast<const double2*>(pp + 64 + l);
                        const double2 pe = *reinterpret_cast<const double2*>(pp + 128 + l);
                        sr += pr.x + pr.y;
                        si += pi.x + pi.y;
                        se += pe.x + pe.y;
                    }
                    const int64_t s = o0 + og + v * ZS_RG + sl;
                    if (live && cx.stored(a, s)) {
                        const double den = te2 * se;
                        out[s] = (OUT)(fma(sr, sr, si * si) / (den > 1e-12 ? den : 1e-12));
                    }
                }
                wave_sync();
            }
        }
        return;
    }
    // steps u, u + 1 reduced together (row_sum2): the lower half of the row ends with step u, the upper
    // half with u + 1, so lane (hi, pos) keeps the steps 2(pos + HALF·j) + hi of the group
    // STEPS consecutive steps reduced together (row_sum2 / row_sum4): lane (which, pos) of the row ends
    // with step u + which and keeps the steps STEPS·(pos + SPAN·j) + which of the group
    constexpr int STEPS = LPC == 16 ? 4 : 2, SPAN = LPC / STEPS, KEEP = ZS_G / LPC;
    const int which = sl / SPAN, pos = sl % SPAN;
    for (int og = 0; og < C; og += ZS_G) {
        zs_stage_d<NB, LPC, ROWS>(a, cx, dbuf, o0, og, live, row, sl);
        wave_sync();
        double keep_n[KEEP], keep_e[KEEP];
#pragma unroll
        for (int j = 0; j < KEEP; ++j) { keep_n[j] = 0.0; keep_e[j] = 0.0; }
#pragma unroll 1
        for (int u = 0; u < ZS_G; u += STEPS) {
            double cr, ci, e;
            if constexpr (STEPS == 4) {
                double cr0, ci0, e0, cr1, ci1, e1, cr2, ci2, e2, cr3, ci3, e3;
                step_terms(g, h, cr0, ci0, e0);
                advance(g, h, u);
                step_terms(h, g, cr1, ci1, e1);
                advance(h, g, u + 1);
                step_terms(g, h, cr2, ci2, e2);
                advance(g, h, u + 2);
                step_terms(h, g, cr3, ci3, e3);
                advance(h, g, u + 3);
                cr = row_sum4(cr0, cr1, cr2, cr3);
                ci = row_sum4(ci0, ci1, ci2, ci3);
                e = row_sum4(e0, e1, e2, e3);
            } else {
                double cr0, ci0, e0, cr1, ci1, e1;
                step_terms(g, h, cr0, ci0, e0);
                advance(g, h, u);
                step_terms(h, g, cr1, ci1, e1);
                advance(h, g, u + 1);
                cr = row_sum2<LPC>(cr0, cr1);
                ci = row_sum2<LPC>(ci0, ci1);
                e = row_sum2<LPC>(e0, e1);
            }
            const double n2 = fma(cr, cr, ci * ci);
#pragma unroll
            for (int j = 0; j < KEEP; ++j)
                if (u / STEPS == pos + SPAN * j) { keep_n[j] = n2; keep_e[j] = e; }
        }
        wave_sync();
#pragma unroll
        for (int j = 0; j < KEEP; ++j) {
            const int64_t s = o0 + og + STEPS * (pos + SPAN * j) + which;
            if (live && cx.stored(a, s)) {
                const double den = te2 * keep_e[j];
                out[s] = (OUT)(keep_n[j] / (den > 1e-12 ? den : 1e-12));
            }
        }
    }
