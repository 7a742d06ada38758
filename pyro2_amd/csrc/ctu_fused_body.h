// The body of the CTU tile kernel behind its prologue (comp_fused.hip): the six phases of one tile's
// step.  Included -- as text, so that every instance compiles from the tokens it always had -- into
// k_ctu_fused and k_ctu_fused_batch, whose prologues differ in where the arguments come from.  In
// scope at the include: SOLVER, STD, NA, NV, NAX; lds; Uin, Uout (old and new level), g, P (with this
// step's dt), flag, partial; blockIdx.x is the tile's number in the launch.
    double *B0 = lds;                 // Q (phase 0-1) | FT (2-3) | F (4-5): x planes, then y planes
    double *S = lds + fbuf0(NA);      // upper face states XP(0..NV-1), YP(NV..2 NV-1)
    double *SY = S + NV * FNT;
    double *BY = B0 + NV * FNT;       // the y fluxes
    double *D = S + 2 * NV * FNT;     // vertex div(U)

    // (a walk that keeps every XCD on a contiguous band of tiles for ANY tile
    // count -- xcd_tile falls back to the identity when it is not divisible by
    // 8, as at 8192^2 and 16384^2 -- and goes through super-columns of 8..64
    // tiles was measured: 3.85 vs 3.82 ms at 8192^2.  The apron re-reads are
    // served by the MALL; phase 0 is bound by latency, not by fabric traffic.)
    const int tile = xcd_tile(blockIdx.x, P.ntiles);
    const int i0 = g.ilo + (tile / P.ntj) * FTI;
    const int j0 = g.jlo + (tile % P.ntj) * FTJ;
    const int tj = threadIdx.x, ti = threadIdx.y;
    const int t = ti * FBJ + tj;
    const int i = i0 - 1 + ti, j = j0 - 1 + tj;
    const int p = g.pitch;
    const size_t pl = g.plane;
    const double gamma = P.gamma;

    // ---- phase 0: U -> Q (rho,u,v,p) for the tile + 4-cell apron --------
    // All global loads of the thread (2 cells x 4 planes) are issued before the
    // first use and the conversion is branch-free: with the `if (U.d != 0)` of
    // cons_to_prim the compiler sank the loads of E, mx, my into the branch, so
    // a workgroup went through four dependent HBM round trips here (density,
    // rest, density, rest) instead of one.
    bool bad = false;
    {
        constexpr int NIT = (FQN + FNT - 1) / FNT;
        Cons Ul[NIT];
        double Al[NIT][NAX];
        bool act[NIT], interior[NIT];
#pragma unroll
        for (int n = 0; n < NIT; n++) {
            const int idx = t + n * FNT;
            act[n] = idx < FQN;
            const int ii = act[n] ? idx : t;       // idle lanes re-read their first cell
            const int r = ii / FQW, c = ii - r * FQW;
            int gi = i0 - 4 + r, gj = j0 - 4 + c;
            const bool inarr = act[n] && gi < g.qx && gj < g.qy;
            gi = (gi < g.qx) ? gi : g.qx - 1;   // ragged last tiles: clamp, unused
            gj = (gj < g.qy) ? gj : g.qy - 1;
            // ghost cells: the cell the boundary rule copies from (itself without
            // fuse_fill), with the sign of reflect-odd variables -- the value
            // fill_BC_all would have stored (x fill, then y fill: both maps)
            unsigned sd;
            const Cons U = load_cons_bc(Uin, g, P, gi, gj, sd);
            Ul[n] = U;
            interior[n] = (sd == 0);
            if constexpr (NA > 0) {
#pragma unroll
                for (int a = 0; a < NA; a++) Al[n][a] = load_aux_bc(Uin, g, P, gi, gj, a);
            }
            // the ghost frame of the new state: what the old state's ghost cells hold
            // (after the fill, when it is folded in) -- as in the reference, where the
            // update leaves the ghost cells of the array alone.  Tiles whose aprons
            // overlap write the same values.
            if (inarr && sd != 0) {
                const size_t ko = (size_t)gi * p + gj;
                Uout[ko] = U.d; Uout[pl + ko] = U.E; Uout[2 * pl + ko] = U.mx; Uout[3 * pl + ko] = U.my;
                if constexpr (NA > 0) {
#pragma unroll
                    for (int a = 0; a < NA; a++) Uout[(4 + a) * pl + ko] = Al[n][a];
                }
            }
        }
#pragma unroll
        for (int n = 0; n < NIT; n++) {
            const int idx = t + n * FNT;
            Cons U = Ul[n];
            const bool dnan = nan_bits(U.d);      // np.maximum keeps a NaN: the floor must not launder it
            if (interior[n]) U.d = fmax(U.d, P.small_dens);      // clean_state
            bool ok;
            const Prim q = cons_to_prim_nb(U, gamma, ok);
            if (act[n] && interior[n] && (!ok || dnan)) bad = true;
            if (act[n]) {
                B0[idx] = q.r; B0[FQN + idx] = q.u; B0[2 * FQN + idx] = q.v; B0[3 * FQN + idx] = q.p;
                if constexpr (NA > 0) {   // X = rho X / rho, the floored rho (simulation.py:75-78)
#pragma unroll
                    for (int a = 0; a < NA; a++) B0[(4 + a) * FQN + idx] = pdiv(Al[n][a], U.d);
                }
            }
        }
    }
    if (bad) atomicOr(flag, 1);
    __syncthreads();
    PYRO_PHASE_END(0, B0[(ti + 3) * FQW + (tj + 3)] + B0[3 * FQN + (ti + 3) * FQW + (tj + 3)])

    // ---- phase 1: xi, slopes, tracing for the thread's own cell --------
    Cons XM, XP, YM, YP;
    double aXM[NAX], aXP[NAX], aYM[NAX], aYP[NAX];   // ... of the scalars
    {
        const int qc = (ti + 3) * FQW + (tj + 3);   // own cell in the Q tile
        const double *Qr = B0, *Qu = B0 + FQN, *Qv = B0 + 2 * FQN, *Qp = B0 + 3 * FQN;
        double xi = 1.0;
        if (STD || P.use_flattening) {
            // flatten_multid (reconstruction.py:167-183): own coefficient and
            // the one of the UPWIND neighbour (w.r.t. the pressure gradient)
            // in each direction -- the downwind one is never selected
            const int sx = (Qp[qc + FQW] - Qp[qc - FQW] > 0) ? -FQW : FQW;
            const int sy = (Qp[qc + 1] - Qp[qc - 1] > 0) ? -1 : 1;
            const int cx = qc + sx, cy = qc + sy;
            const double xix = flatten_1d(Qp[qc - 2 * FQW], Qp[qc - FQW], Qp[qc + FQW],
                                          Qp[qc + 2 * FQW], Qu[qc - FQW], Qu[qc + FQW], P.z0, P.z1,
                                          P.delta);
            const double px = flatten_1d(Qp[cx - 2 * FQW], Qp[cx - FQW], Qp[cx + FQW],
                                         Qp[cx + 2 * FQW], Qu[cx - FQW], Qu[cx + FQW], P.z0, P.z1,
                                         P.delta);
            const double xiy = flatten_1d(Qp[qc - 2], Qp[qc - 1], Qp[qc + 1], Qp[qc + 2],
                                          Qv[qc - 1], Qv[qc + 1], P.z0, P.z1, P.delta);
            const double py = flatten_1d(Qp[cy - 2], Qp[cy - 1], Qp[cy + 1], Qp[cy + 2],
                                         Qv[cy - 1], Qv[cy + 1], P.z0, P.z1, P.delta);
            xi = fmin(fmin(xix, px), fmin(xiy, py));
        }
        double q0[NV], dqx[NV], dqy[NV];
#pragma unroll
        for (int n = 0; n < NV; n++) {
            const double *a = B0 + n * FQN;
            q0[n] = a[qc];
            dqx[n] = xi * limited_slope(a[qc - 2 * FQW], a[qc - FQW], a[qc], a[qc + FQW],
                                        a[qc + 2 * FQW], STD ? 2 : P.limiter);
            dqy[n] = xi * limited_slope(a[qc - 2], a[qc - 1], a[qc], a[qc + 1], a[qc + 2],
                                        STD ? 2 : P.limiter);
        }
        Trace lo, hi;
        trace_states(q0[0], q0[1], q0[2], q0[3], dqx[0], dqx[1], dqx[2], dqx[3], gamma,
                     P.dtdx, lo, hi);
        XM = prim_to_cons(Prim{lo.r, lo.un, lo.ut, lo.p}, gamma);
        XP = prim_to_cons(Prim{hi.r, hi.un, hi.ut, hi.p}, gamma);
        trace_states(q0[0], q0[2], q0[1], q0[3], dqy[0], dqy[2], dqy[1], dqy[3], gamma,
                     P.dtdy, lo, hi);
        YM = prim_to_cons(Prim{lo.r, lo.ut, lo.un, lo.p}, gamma);
        YP = prim_to_cons(Prim{hi.r, hi.ut, hi.un, hi.p}, gamma);
        if constexpr (NA > 0) {
            // the scalars' face states: traced with the fluid, then rho X = X rho of the face state
            // (prim_to_cons, simulation.py:101-104); no source term touches them
#pragma unroll
            for (int a = 0; a < NA; a++) {
                double xl, xh;
                trace_passive(q0[0], q0[1], q0[3], q0[4 + a], dqx[4 + a], gamma, P.dtdx, xl, xh);
                aXM[a] = aux_keep(xl * XM.d); aXP[a] = aux_keep(xh * XP.d);
                trace_passive(q0[0], q0[2], q0[3], q0[4 + a], dqy[4 + a], gamma, P.dtdy, xl, xh);
                aYM[a] = aux_keep(xl * YM.d); aYP[a] = aux_keep(xh * YP.d);
            }
        }
        // vertex divergence at (i-1/2, j-1/2), interface.py:312-330
        D[t] = div_u_vertex(Qu[qc], Qu[qc - 1], Qu[qc - FQW], Qu[qc - FQW - 1], Qv[qc],
                            Qv[qc - FQW], Qv[qc - 1], Qv[qc - FQW - 1], P.dx, P.dy);
        if (P.have_src) {   // apply_source_terms, unsplit_fluxes.py:247-330
            const bool ina = (i < g.qx && j < g.qy);
            // "ambient" upper boundary: the source ghosts are copies of row jhi
            // (BC.py:159-160), not the sources of the ambient ghost state
            const int js = (P.amb_yhi && j > g.jhi) ? g.jhi : j;
            const size_t kc = (size_t)(ina ? i : g.qx - 1) * p + (ina ? js : g.qy - 1);
            Cons Ug{Uin[kc], 0.0, 0.0, Uin[3 * pl + kc]};
            if (i >= g.ilo && i <= g.ihi && js >= g.jlo && js <= g.jhi)
                Ug.d = fmax(Ug.d, P.small_dens);
            else Ug.d = ghost_src_dens(Ug.d, P.small_dens);
            const double sgn =
                ((j < g.jlo && P.refl_ylo) || (j > g.jhi && P.refl_yhi)) ? -1.0 : 1.0;
            const double hp = P.heat ? P.heat[(size_t)(ina ? i : g.qx - 1) * p + (ina ? j : g.qy - 1)]
                                     : 0.0;
            add_grav_to_state(XM, Ug, P.grav, P.dt, sgn, P.heat_rate, hp);
            add_grav_to_state(XP, Ug, P.grav, P.dt, sgn, P.heat_rate, hp);
            add_grav_to_state(YM, Ug, P.grav, P.dt, sgn, P.heat_rate, hp);
            add_grav_to_state(YP, Ug, P.grav, P.dt, sgn, P.heat_rate, hp);
        }
        lds_put(S, t, XP);
        lds_put(SY, t, YP);
        if constexpr (NA > 0) {
#pragma unroll
            for (int a = 0; a < NA; a++) { S[(4 + a) * FNT + t] = aXP[a]; SY[(4 + a) * FNT + t] = aYP[a]; }
        }
    }
    __syncthreads();   // Q is dead from here on; B0 becomes the flux buffer
    PYRO_PHASE_END(1, XM.d + XM.E + XM.mx + XM.my + YM.d + YM.E + YM.mx + YM.my + S[t] + S[7 * FNT + t] + D[t])

    // ---- phase 2: transverse Riemann problems on the lower faces --------
    Cons FxT{0, 0, 0, 0}, FyT{0, 0, 0, 0};
    double aFxT[NAX] = {}, aFyT[NAX] = {};
    if (ti >= 1)
        FxT = face_flux<SOLVER, NA>(S, t - FBJ, XM, aXM, gamma, true, P.solid_xl && i == g.ilo, aFxT);
    if (tj >= 1)
        FyT = face_flux<SOLVER, NA>(SY, t - 1, YM, aYM, gamma, false, P.solid_yl && j == g.jlo, aFyT);
    lds_put(B0, t, FxT);
    lds_put(BY, t, FyT);
    if constexpr (NA > 0) {
#pragma unroll
        for (int a = 0; a < NA; a++) { B0[(4 + a) * FNT + t] = aFxT[a]; BY[(4 + a) * FNT + t] = aFyT[a]; }
    }
    __syncthreads();
    PYRO_PHASE_END(2, FxT.d + FxT.E + FxT.mx + FxT.my + FyT.d + FyT.E + FyT.mx + FyT.my + XM.d + YM.E)

    // ---- phase 3: transverse correction of the cell's own states --------
    const double hdtV = P.hdtV;                          // hdt / V
    const double Ax = P.dy, Ay = P.dx;
    if (tj >= 1 && tj <= FBJ - 2) {
        const Cons Fhi = lds_get(BY, t + 1);             // F_yT at (i, j+1)
        XM = corr(XM, Fhi, FyT, hdtV, Ay);
        XP = corr(XP, Fhi, FyT, hdtV, Ay);
        if constexpr (NA > 0) {
#pragma unroll
            for (int a = 0; a < NA; a++) {
                const double fh = BY[(4 + a) * FNT + t + 1];
                aXM[a] = corr1(aXM[a], fh, aFyT[a], hdtV, Ay);
                aXP[a] = corr1(aXP[a], fh, aFyT[a], hdtV, Ay);
            }
        }
    }
    if (ti >= 1 && ti <= FBI - 2) {
        const Cons Fhi = lds_get(B0, t + FBJ);           // F_xT at (i+1, j)
        YM = corr(YM, Fhi, FxT, hdtV, Ax);
        YP = corr(YP, Fhi, FxT, hdtV, Ax);
        if constexpr (NA > 0) {
#pragma unroll
            for (int a = 0; a < NA; a++) {
                const double fh = B0[(4 + a) * FNT + t + FBJ];
                aYM[a] = corr1(aYM[a], fh, aFxT[a], hdtV, Ax);
                aYP[a] = corr1(aYP[a], fh, aFxT[a], hdtV, Ax);
            }
        }
    }
    // (all reads of the uncorrected upper states happened before the barrier
    // that closed phase 2; phase 3 itself only reads the flux buffer)
    lds_put(S, t, XP);
    lds_put(SY, t, YP);
    if constexpr (NA > 0) {
#pragma unroll
        for (int a = 0; a < NA; a++) { S[(4 + a) * FNT + t] = aXP[a]; SY[(4 + a) * FNT + t] = aYP[a]; }
    }
    __syncthreads();
    PYRO_PHASE_END(3, XM.d + XM.E + XM.mx + XM.my + YM.d + YM.E + YM.mx + YM.my + S[t] + S[7 * FNT + t])

    // ---- phase 4: final Riemann problems + artificial viscosity ---------
    const bool in_arr = (i < g.qx && j < g.qy);
    const int ic = in_arr ? i : g.qx - 1, jc = in_arr ? j : g.qy - 1;
    const size_t k = (size_t)ic * p + jc;
    unsigned sdc;
    Cons Uc = load_cons_bc(Uin, g, P, ic, jc, sdc);
    const bool cell_interior = (i >= g.ilo && i <= g.ihi && j >= g.jlo && j <= g.jhi);
    if (cell_interior) Uc.d = fmax(Uc.d, P.small_dens);
    Cons Fx{0, 0, 0, 0}, Fy{0, 0, 0, 0};
    const double d00 = D[t];
    // the lower neighbours' old states for the artificial-viscosity terms:
    // loaded (L2 hits) before the Riemann problems so that the latency is
    // covered by them.  k - p / k - 1 are inside the array for every thread.
    Cons Umx = load_cons_bc(Uin, g, P, ic - 1, jc, sdc);
    Cons Umy = load_cons_bc(Uin, g, P, ic, jc - 1, sdc);
    double aUc[NAX], aUmx[NAX], aUmy[NAX], aFx[NAX] = {}, aFy[NAX] = {};
    if constexpr (NA > 0) {
#pragma unroll
        for (int a = 0; a < NA; a++) {
            aUc[a] = load_aux_bc(Uin, g, P, ic, jc, a);
            aUmx[a] = load_aux_bc(Uin, g, P, ic - 1, jc, a);
            aUmy[a] = load_aux_bc(Uin, g, P, ic, jc - 1, a);
        }
    }
    double avx = 0.0, avy = 0.0;
    // interface.py:366-376: only faces i in [ilo, ihi], j in [jlo, jhi]
    if (ti >= 1 && tj >= 1 && tj <= FBJ - 2 && i >= g.ilo &&
        (i <= g.ihi || (P.avx_hi && i == g.ihi + 1)) && j >= g.jlo && j <= g.jhi) {
        const double divU_x = 0.5 * (d00 + D[t + 1]);
        avx = P.cvisc * fmax(-divU_x * P.dx, 0.0);
    }
    if (tj >= 1 && ti >= 1 && ti <= FBI - 2 && j >= g.jlo &&
        (j <= g.jhi || (P.avy_hi && j == g.jhi + 1)) && i >= g.ilo && i <= g.ihi) {
        const double divU_y = 0.5 * (d00 + D[t + FBJ]);
        avy = P.cvisc * fmax(-divU_y * P.dy, 0.0);
    }
    if (i - 1 >= g.ilo && i - 1 <= g.ihi && j >= g.jlo && j <= g.jhi)
        Umx.d = fmax(Umx.d, P.small_dens);
    if (i >= g.ilo && i <= g.ihi && j - 1 >= g.jlo && j - 1 <= g.jhi)
        Umy.d = fmax(Umy.d, P.small_dens);
    if (ti >= 1 && tj >= 1 && tj <= FBJ - 2) {           // x face (i, j)
        Fx = face_flux<SOLVER, NA>(S, t - FBJ, XM, aXM, gamma, true, P.solid_xl && i == g.ilo, aFx);
        Fx.d += avx * (Umx.d - Uc.d);
        Fx.E += avx * (Umx.E - Uc.E);
        Fx.mx += avx * (Umx.mx - Uc.mx);
        Fx.my += avx * (Umx.my - Uc.my);
        if constexpr (NA > 0) {
#pragma unroll
            for (int a = 0; a < NA; a++) aFx[a] = avisc1(aFx[a], avx, aUmx[a], aUc[a]);
        }
    }
    if (tj >= 1 && ti >= 1 && ti <= FBI - 2) {           // y face (i, j)
        Fy = face_flux<SOLVER, NA>(SY, t - 1, YM, aYM, gamma, false, P.solid_yl && j == g.jlo, aFy);
        Fy.d += avy * (Umy.d - Uc.d);
        Fy.E += avy * (Umy.E - Uc.E);
        Fy.mx += avy * (Umy.mx - Uc.mx);
        Fy.my += avy * (Umy.my - Uc.my);
        if constexpr (NA > 0) {
#pragma unroll
            for (int a = 0; a < NA; a++) aFy[a] = avisc1(aFy[a], avy, aUmy[a], aUc[a]);
        }
    }
    lds_put(B0, t, Fx);            // FT was last read before the barrier above
    lds_put(BY, t, Fy);
    if constexpr (NA > 0) {
#pragma unroll
        for (int a = 0; a < NA; a++) { B0[(4 + a) * FNT + t] = aFx[a]; BY[(4 + a) * FNT + t] = aFy[a]; }
    }
    __syncthreads();
    PYRO_PHASE_END(4, Fx.d + Fx.E + Fx.mx + Fx.my + Fy.d + Fy.E + Fy.mx + Fy.my)

    // ---- phase 5: conservative update + CFL of the new state -----------
    double cfl = INFINITY;
    if (ti >= 1 && ti <= FBI - 2 && tj >= 1 && tj <= FBJ - 2 && cell_interior) {
        const double dtdV = P.dtdV;
        const Cons Fxh = lds_get(B0, t + FBJ);
        const Cons Fyh = lds_get(BY, t + 1);
        Cons Un;   // simulation.py:377-384
        Un.d = Uc.d + dtdV * (Fx.d * Ax - Fxh.d * Ax + Fy.d * Ay - Fyh.d * Ay);
        Un.E = Uc.E + dtdV * (Fx.E * Ax - Fxh.E * Ax + Fy.E * Ay - Fyh.E * Ay);
        Un.mx = Uc.mx + dtdV * (Fx.mx * Ax - Fxh.mx * Ax + Fy.mx * Ay - Fyh.mx * Ay);
        Un.my = Uc.my + dtdV * (Fx.my * Ax - Fxh.my * Ax + Fy.my * Ay - Fyh.my * Ay);
        if (P.have_src)   // simulation.py:406-423
            grav_update(Un, Uc, P.grav, P.dt, P.heat_rate, P.heat ? P.heat[k] : 0.0);
        Uout[k] = Un.d; Uout[pl + k] = Un.E; Uout[2 * pl + k] = Un.mx; Uout[3 * pl + k] = Un.my;
        if constexpr (NA > 0) {   // the same update; no source term, and the CFL minimum is the hydro one
#pragma unroll
            for (int a = 0; a < NA; a++) {
                const double fxh = B0[(4 + a) * FNT + t + FBJ], fyh = BY[(4 + a) * FNT + t + 1];
                Uout[(4 + a) * pl + k] = update1(aUc[a], dtdV, aFx[a], fxh, Ax, aFy[a], fyh, Ay);
            }
        }
        cfl = cfl_cell(Un, gamma, P.dx, P.dy);
    }
    cfl = block_reduce_min(cfl);
    if (t == 0) partial[tile] = cfl;
