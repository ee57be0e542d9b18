// lf_fused_level_steps.inc -- the body of the time-major level kernels of lf_fused.h (see the comment above
// k_fused_level_steps there), included once by each of them: k_fused_level_steps and k_fused_level_steps_members.  It expects
// in scope: F (fused_args), k (the level), and the compile-time constants SPLIT, ALL35, DIST and STRUCT.
// (A text and not a function: as a __forceinline__ function called by both kernels the sub-step loop came out of the compiler
// with another instruction stream in every existing instantiation -- DESIGN.md section 4.2b.)
    static_assert(!(DIST && STRUCT != 0), "the row-block partition runs no structures");
    const lf_substep_args &A = F.S;
    // (STRUCT = 2: lane i works on the i-th site of level k, the cell is that site's)
    const long long first = STRUCT == 2 ? (long long)F.tm_site_ptr[k] : F.level_start[k];
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (STRUCT == 2 ? (long long)F.tm_site_ptr[k + 1] : F.level_start[k + 1]) - first) return;
    const long long site = STRUCT == 2 ? (long long)F.tm_site[first + i] : 0;
    const long long p = STRUCT == 2 ? (long long)(site < F.I.n_lakes ? F.I.lake_cell[site] : F.I.res_cell[site - F.I.n_lakes]) : first + i,
                    n = F.n;
    const int nsteps = F.nsteps;
    const int u0 = F.ups_ptr[p], u1 = F.ups_ptr[p + 1], kmax = F.kmax;
    int base = u0;
    long long slot = -1;
    if (DIST) {
        // (a run of ghost slots is not a local run, and a local run with a cell of another phase has no base: see
        // k_fused_substeps<DIST>)
        const int base_raw = F.d_ups_base[p];
        base = (base_raw >= 0 && (long long)base_raw + (u1 - u0) <= n) ? base_raw : -1;
        slot = F.d_out_slot[p];
    }
    auto ups_of = [&](const double *hist, const double *slab, int s) {
        if (!DIST) return upstream_sum8_pairs(hist + (long long)s * n, u0, u1, kmax);
        if (base >= 0) return upstream_sum8(hist + (long long)s * n, base, base + (u1 - u0), kmax);
        double v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            double x = 0.0;
            if (j < kmax && u0 + j < u1) {
                const int e = F.d_ups_idx[u0 + j];
                x = e >= 0 ? hist[(long long)s * n + e] : slab[(long long)(-(e + 1)) * F.root_ss + (long long)s * F.root_st];
            }
            v[j] = x;
        }
        double ups = 0.0;
#pragma unroll
        for (int j = 0; j < 8; ++j) ups += v[j];
        return ups;
    };
    const bool b35 = A.Beta == 0.6, s35 = F.solve35 != 0;
    const unsigned int dflags = derived_flags(F);
    const bool rc = (dflags & 1u) != 0u;
    const double len = A.ChanLength[p];
    const double dxp = (dflags & 2u) ? len : (F.dx ? F.dx[p] : F.dx_scalar);
    const double inv_len = rc ? 1.0 / len : A.InvChanLength[p];
    const bool is_chan = A.IsChannelKinematic[p] != 0;
    bool cut;
    int feed = -1; // STRUCT = 1: this cell's row entry in the feed buffer
    if constexpr (STRUCT != 0) {
        const unsigned fl = F.linked ? F.linked[p] : 0u;
        if (STRUCT == 1 && (fl & 2u)) return; // a site cell: run by the site lanes behind this launch
        cut = (fl & 1u) != 0u;
        if (STRUCT == 1 && cut && F.tm_slot) feed = F.tm_slot[p];
    } else
        cut = F.linked && F.linked[p];
    const double alpha1 = A.ChannelAlpha[p];
    const double inv_alpha1 = rc ? 1.0 / alpha1 : A.InvChannelAlpha[p], ap1 = rc ? alpha1 * dxp / F.dt : F.a1[p];
    double qold = A.ChanQKin[p], sum = 0.0;
    double m3 = 0, m3_2 = 0, start = 0, m3limit = 0, q2start = 0, ap2 = 0, q2old = 0, alpha2 = 0, inv_alpha2 = 0, qlimit = 0;
    if (SPLIT) {
        m3 = A.ChanM3Kin[p];
        m3_2 = A.Chan2M3Kin[p];
        start = A.Chan2M3Start[p];
        m3limit = A.M3Limit[p];
        q2start = A.Chan2QStart[p];
        q2old = A.Chan2QKin[p];
        alpha2 = A.ChannelAlpha2[p];
        ap2 = rc ? alpha2 * dxp / F.dt : F.a2[p];
        inv_alpha2 = rc ? 1.0 / alpha2 : A.InvChannelAlpha2[p];
        qlimit = A.QLimit[p];
    }
    const double pix_area = A.PixelArea[p];
    int s0 = 0;
    if (STRUCT == 0 && F.inert && F.inert[p]) { // see k_inert_flags: a sub-step leaves such a cell as it is while its state is all +0.0,
                                 // so only the last one (which also writes the velocities) is run, as fused_cell does
        bool zero = plus_zero(qold) && plus_zero(A.ChanM3Kin[p]) && plus_zero(A.ChanQ[p]);
        if (SPLIT && zero)
            zero = plus_zero(q2old) && plus_zero(m3_2) && plus_zero(A.CrossSection2Area[p]) && plus_zero(A.Sideflow1Chan[p]);
        if (zero) {
            s0 = nsteps - 1;
            // several model steps in the call: fused_cell runs the last sub-step of EVERY model step on such a cell and
            // stores sum + ChanQ with ChanQ = +0.0 -- the same store here, so that a -0.0 the caller left in the sums of
            // the earlier model steps ends up as +0.0 in both forms (any other value is unchanged by the addition)
            for (int m = F.msteps - 1; m < nsteps - 1; m += F.msteps) fused_sum(F, m)[p] = fused_sum(F, m)[p] + 0.0;
        }
    }
    double v = 0, q = 0, chanq = 0, s1 = 0, v2 = 0, q2 = 0;
    double side_m3 = STRUCT != 0 ? 0.0 : fused_side(F, s0)[p];
    // STRUCT: the terms of the sideflow assembly (routing.py:462-478) and what the loop carries from sub-step to sub-step
    double to_chan = 0, eva = 0, wuse = 0, qin_old = 0, qdelta = 0, qin = 0, qin_added = 0.0, loss = 0, trans_cum = 0, lakeout = 0,
           resout = 0, polder = 0;
    bool uptrans = false;
    int res_slot0 = 0; // STRUCT = 2: first feed slot of the reservoirs' lists
    if constexpr (STRUCT != 0) {
        const lf_inloop_args &I = F.I;
        to_chan = I.ToChanM3RunoffDt[p];
        if (I.EvaAddM3Dt) eva = I.EvaAddM3Dt[p];
        if (I.WUseAddM3Dt) wuse = I.WUseAddM3Dt[p];
        if (I.QInM3Old) {
            qin_old = I.QInM3Old[p];
            qdelta = I.QDelta[p];
        }
        if (I.UpTrans) {
            uptrans = I.UpTrans[p] != 0;
            trans_cum = I.TransCum[p];
        }
        if (I.QLakeOutM3Dt) lakeout = I.QLakeOutM3Dt[p];
        if (I.QResOutM3Dt) resout = I.QResOutM3Dt[p];
        if (I.ChannelToPolderM3Dt) polder = I.ChannelToPolderM3Dt[p];
        chanq = A.ChanQ[p]; // ChanQ before the first sub-step: transmission loss, the sites' inflow
        if (STRUCT == 1 && feed >= 0) F.tm_feed[feed] = chanq;
        if (STRUCT == 2 && I.n_lakes > 0) res_slot0 = I.lake_ups_ptr[I.n_lakes];
    }
    sum = fused_sum(F, s0)[p];
    // position of the sub-step inside its model step, counted along (s starts per lane -- inert cells run only the last
    // sub-step -- so `s % msteps` would be a vector-register division, ~25 instructions, twice per sub-step)
    int sm = s0 % F.msteps;
    for (int s = s0; s < nsteps; ++s) {
        double ups1, ups2;
        if (!DIST) {
            upstream_sum8_pairs2(F.hist1 + (long long)s * n, F.hist2 + (long long)s * n, SPLIT, u0, u1, kmax, ups1, ups2);
        } else {
            ups1 = ups_of(F.hist1, F.root1, s);
            ups2 = SPLIT ? ups_of(F.hist2, F.root2, s) : 0.0;
        }
        const bool first_of_step = sm == 0;
        if constexpr (STRUCT == 0) {
            if ((F.side_stride != 0 || first_of_step) && s > s0) side_m3 = fused_side(F, s)[p];
        } else { // inflow.py:142-144, transmission.py:76-87, sideflow assembly routing.py:462-478 -- as fused_cell<STRUCT>
            const lf_inloop_args &I = F.I;
            if constexpr (STRUCT == 2) { // the site first: its feeders' ChanQ after sub-step s - 1, ascending list order
                const double *row = F.tm_feed + (long long)s * F.tm_nfeed;
                double inflow = 0.0;
                if (site < I.n_lakes) {
                    for (int e = I.lake_ups_ptr[site]; e < I.lake_ups_ptr[site + 1]; ++e) inflow += row[e];
                } else {
                    const long long r = site - I.n_lakes;
                    for (int e = I.res_ups_ptr[r]; e < I.res_ups_ptr[r + 1]; ++e) inflow += row[res_slot0 + e];
                }
                lf_site_body(I, site, inflow);
                if (I.QLakeOutM3Dt) lakeout = I.QLakeOutM3Dt[p];
                if (I.QResOutM3Dt) resout = I.QResOutM3Dt[p];
            }
            side_m3 = to_chan;
            if (I.EvaAddM3Dt) side_m3 -= eva;
            if (I.WUseAddM3Dt) side_m3 -= wuse;
            if (I.QInM3Old) {
                qin = (qin_old + (s + 1) * qdelta) * I.InvNoRoutSteps;
                qin_added = qin_added + qin; // (sub-step 0: 0.0 + qin)
                side_m3 += qin;
            }
            if (I.UpTrans) {
                const double qc = chanq;
                const double tout = uptrans ? lf_pow_scalar_exponent(lf_pow_scalar_exponent(qc, I.TransPower2) - I.TransSub, I.TransPower1) : qc;
                loss = (qc - tout) * I.DtRouting;
                trans_cum = trans_cum + loss;
                side_m3 -= loss;
            }
            if (I.QLakeOutM3Dt) side_m3 += lakeout;
            if (I.QResOutM3Dt) side_m3 += resout;
            if (I.ChannelToPolderM3Dt) side_m3 -= polder;
        }
        if (first_of_step && s > s0) sum = fused_sum(F, s)[p]; // the next model step's sum (zeroed by the caller)
        // ---- sideflow (routing.py:512, 524 / 549-567) ----
        const double side = is_chan ? side_m3 * inv_len * A.InvDtRouting : 0.0;
        double s2 = 0.0;
        s1 = side;
        if (!SPLIT) {
            if (isnan(side)) s1 = 0.0;
        } else {
            const double tot = m3 + m3_2;
            const double ratio = (tot > 0) ? m3 / tot : 0.0;
            s1 = ((tot - start) > m3limit) ? ratio * side : side;
            if (fabs(side) < 1e-7) s1 = side;
            s2 = (side - s1) + q2start * inv_len;
        }
        // ---- main channel: router call + fix-up (routing.py:526-532 / 573-578); floodplains (routing.py:583-603) ----
        double qr, q2r = 0;
        if constexpr (ALL35) {
            double pw1, pw2, pr1, pr2;
            cone_pow_3_5_two<SPLIT>(qold, q2old, pw1, pw2);
            const double c = ups1 + (ap1 * pw1 + s1 * dxp);
            const double c2 = SPLIT ? ups2 + (ap2 * pw2 + s2 * dxp) : 0.0;
            cone_solve_two<SPLIT>(c, ap1, c2, ap2, F, qr, q2r);
            cone_pow_3_5_two<SPLIT>(qr, q2r, pr1, pr2);
            v = len * alpha1 * pr1;
            if (v < 0.0) v = 0.0;
            const double x = v * inv_len * inv_alpha1;
            double x2 = 0.0;
            if (SPLIT) {
                v2 = len * alpha2 * pr2;
                if ((v2 - start) < 0.0) v2 = start;
                x2 = v2 * inv_len * inv_alpha2;
            }
            cone_pow_5_3_two<SPLIT>(x, x2, q, q2);
            chanq = q;
            if (SPLIT) {
                chanq = q + q2 - qlimit;
                if (chanq < 0.0) chanq = 0.0;
            }
        } else {
            const double cst = ap1 * (s35 ? lf_pow_3_5(qold) : pow(qold, F.beta)) + s1 * dxp;
            const double c = ups1 + cst;
            qr = solve_any(c, ap1, s35, F);
            v = len * alpha1 * (b35 ? lf_pow_3_5(qr) : pow(qr, A.Beta));
            if (v < 0.0) v = 0.0;
            const double x = v * inv_len * inv_alpha1;
            q = b35 ? lf_pow_5_3(x) : pow(x, A.InvBeta);
            chanq = q;
            if (SPLIT) {
                const double cst2 = ap2 * (s35 ? lf_pow_3_5(q2old) : pow(q2old, F.beta)) + s2 * dxp;
                const double c2 = ups2 + cst2;
                q2r = solve_any(c2, ap2, s35, F);
                v2 = len * alpha2 * (b35 ? lf_pow_3_5(q2r) : pow(q2r, A.Beta));
                if ((v2 - start) < 0.0) v2 = start;
                const double x2 = v2 * inv_len * inv_alpha2;
                q2 = b35 ? lf_pow_5_3(x2) : pow(x2, A.InvBeta);
                chanq = q + q2 - qlimit;
                if (chanq < 0.0) chanq = 0.0;
            }
        }
        F.hist1[(long long)s * n + p] = cut ? 0.0 : qr;
        if (SPLIT) F.hist2[(long long)s * n + p] = cut ? 0.0 : q2r;
        if (DIST && slot >= 0) { // kept for the next phase / rank, as fused_cell does
            F.root1[slot * F.root_ss + (long long)s * F.root_st] = qr;
            if (SPLIT) F.root2[slot * F.root_ss + (long long)s * F.root_st] = q2r;
        }
        if constexpr (STRUCT == 1)
            if (feed >= 0) F.tm_feed[(long long)(s + 1) * F.tm_nfeed + feed] = chanq; // read by the site at sub-step s + 1
        // the state of the next sub-step
        m3 = v;
        qold = q;
        sum = sum + chanq;
        const bool last_of_step = sm + 1 == F.msteps; // fused_last(F, s)
        if (last_of_step && s != nsteps - 1) fused_sum(F, s)[p] = sum; // a model step inside the call is complete
        sm = last_of_step ? 0 : sm + 1;
        if (SPLIT) {
            m3_2 = v2;
            q2old = q2;
        }
    }
    // ---- what the sub-step-by-sub-step sequence leaves behind ----
    if constexpr (STRUCT != 0) {
        const lf_inloop_args &I = F.I;
        if (I.QInM3Old) {
            I.QInDt[p] = qin;
            I.QinADDEDM3[p] = qin_added;
        }
        if (I.UpTrans) {
            I.TransLossM3Dt[p] = loss;
            I.TransCum[p] = trans_cum;
        }
        I.SideflowChanM3[p] = side_m3;
    }
    A.ChanM3Kin[p] = v;
    A.ChanQKin[p] = q;
    A.ChanQ[p] = chanq;
    fused_sum(F, nsteps - 1)[p] = sum;
    if (SPLIT) {
        A.Sideflow1Chan[p] = s1;
        A.Chan2M3Kin[p] = v2;
        A.CrossSection2Area[p] = (v2 - start) * inv_len;
        A.Chan2QKin[p] = q2;
    }
    { // routing.py:693-703
        double area = v * inv_len;
        if (area < 0.01) area = 0.01;
        const double v1 = q / area, vv2 = 0.36 * pow(q, 0.24);
        double vel = (vv2 < v1) ? vv2 : v1;
        if (isnan(vv2)) vel = vv2;
        double sinu = sqrt(pix_area) * inv_len;
        if (sinu > 1) sinu = 1;
        vel *= sinu;
        A.FlowVelocity[p] = vel;
        A.TravelDistance[p] = vel * A.DtSec;
    }
