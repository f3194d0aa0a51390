// world/ccd.hpp -- fragment of the body of `template <class T> struct World` (avn_world.hip includes it inside the class):
// swept CCD (include/avian_mi355x_ccd.h; k_ccd.hip): the SweptCcd list, the pass between the substep loop and the restitution pass of the
// device closed loop, the records of the last pass.  Without a list nothing here launches, stamps or allocates.

    CCD<T> ccd{};
    DevBuf b_ccd_body, b_ccd_incl, b_ccd_lin2, b_ccd_ang2, b_ccd_own, b_ccd_entry, b_ccd_ctr, b_ccd_cand, b_ccd_cand_t, b_ccd_min_t, b_ccd_min_key, b_ccd_rec,
        b_ccd_wkey_a, b_ccd_wval_a, b_ccd_wkey_b, b_ccd_wval_b, b_ccd_hist, b_ccd_sums, b_ccd_mode, b_ccd_bmode;
    bool ccd_nl_on = false;         // avn_swept_ccd_non_linear_set: AVN_SWEEP_NON_LINEAR is accepted (sticky, off in a new world)
    bool ccd_caps_on = false;       // avn_swept_ccd_capsules_set: pairs with an AVN_SHAPE_CAPSULE collider are tested (sticky, off in a new world)
    bool ccd_tables_dirty = true;   // CCD::own / CCD::entry name the collider table of an earlier upload (colliders / collider transforms / the list itself)
    bool ccd_ran = false;           // a pass has run since the list was uploaded
    bool ccd_stamped = false;       // this step's pass recorded ev_ccd
    hipEvent_t ev_ccd = nullptr;    // SolverDiagnostics::swept_ccd: after the pass (it starts at DG_SUB1)

    void ccd_clear() { ccd.n = 0; ccd.mode = nullptr; ccd.body_mode = nullptr; ccd_ran = false; ccd_tables_dirty = true; }
    bool ccd_closed_loop() const { return pipe_on && pipe_dev && !halo_on && !dsh_on; }

    avn_status swept_ccd_upload(const avn_swept_ccd* l) override {
        if (l && l->struct_size != sizeof(avn_swept_ccd)) { error = "swept_ccd_upload: struct_size"; return AVN_ERR_BAD_ARG; }
        if (halo_on || dsh_on) { error = "swept_ccd_upload: not in a level-2 / sharded world"; return AVN_ERR_STATE; }
        if (!l || l->count == 0) { ccd_clear(); return AVN_OK; }
        if (!have_bodies) { error = "swept_ccd_upload: before bodies_upload"; return AVN_ERR_STATE; }
        if (despawn_needs_bodies || despawn_needs_colliders) { error = "swept_ccd_upload: avn_despawn is still waiting for avn_bodies_upload / avn_colliders_upload"; return AVN_ERR_STATE; }
        const uint32_t n = l->count;
        if (!l->body || !l->mode || !l->include_dynamic || !l->linear_threshold || !l->angular_threshold) { error = "swept_ccd_upload: null array"; return AVN_ERR_BAD_ARG; }
        if (n > 0x40000000u) { error = "swept_ccd_upload: too many entries"; return AVN_ERR_BAD_ARG; }
        std::vector<uint8_t> seen(dw.n_bodies, 0);
        bool any_nl = false;
        for (uint32_t i = 0; i < n; ++i) {
            if (l->mode[i] != AVN_SWEEP_LINEAR && !ccd_nl_on) { error = "swept_ccd_upload: SweepMode::NonLinear is not built (only AVN_SWEEP_LINEAR)"; return AVN_ERR_BAD_ARG; }
            if (l->mode[i] > AVN_SWEEP_NON_LINEAR) { error = "swept_ccd_upload: a mode that is neither AVN_SWEEP_LINEAR nor AVN_SWEEP_NON_LINEAR"; return AVN_ERR_BAD_ARG; }
            any_nl = any_nl || l->mode[i] == AVN_SWEEP_NON_LINEAR;
            if (l->body[i] >= dw.n_bodies) { error = "swept_ccd_upload: body index out of range"; return AVN_ERR_BAD_ARG; }
            if (seen[l->body[i]]) { error = "swept_ccd_upload: a body is named twice"; return AVN_ERR_BAD_ARG; }
            seen[l->body[i]] = 1;
        }
        // (the previous list's buffers may still be read by a step in flight)
        HIPCHK(hipStreamSynchronize(stream)); HIPCHK(hipStreamSynchronize(stream_bp));
        std::vector<uint32_t> incl(n);
        std::vector<T> lin2(n), ang2(n);
        for (uint32_t i = 0; i < n; ++i) {
            incl[i] = l->include_dynamic[i] ? 1u : 0u;
            const T lt = (T)l->linear_threshold[i], at = (T)l->angular_threshold[i];
            lin2[i] = lt * lt; ang2[i] = at * at;
        }
        CCD<T> c = ccd;
        ccd_clear();   // (a failure below leaves no list: the old list's buffers may have moved)
        uint32_t *d_body = nullptr, *d_incl = nullptr; T *d_lin2 = nullptr, *d_ang2 = nullptr;
        GROW(b_ccd_body, n, d_body); GROW(b_ccd_incl, n, d_incl); GROW(b_ccd_lin2, n, d_lin2); GROW(b_ccd_ang2, n, d_ang2);
        GROW(b_ccd_own, dw.n_bodies, c.own); GROW(b_ccd_ctr, 16, c.ctr); GROW(b_ccd_min_t, n, c.min_t); GROW(b_ccd_min_key, n, c.min_key); GROW(b_ccd_rec, n, c.rec);
        GROW(b_ccd_wkey_a, 2 * (size_t)n, c.wkey_a); GROW(b_ccd_wval_a, 2 * (size_t)n, c.wval_a); GROW(b_ccd_wkey_b, 2 * (size_t)n, c.wkey_b); GROW(b_ccd_wval_b, 2 * (size_t)n, c.wval_b);
        GROW(b_ccd_hist, (size_t)256 * radix_blocks(2 * n) + 256, c.hist);
        GROW(b_ccd_sums, scan_block_sums_needed(256 * radix_blocks(2 * n)) + 16, c.block_sums);
        // the mode tables exist only for a list with a NonLinear entry; CCD::mode == nullptr is what keeps the _nl kernels from launching
        uint32_t *d_mode = nullptr, *d_bmode = nullptr;
        if (any_nl) {
            GROW(b_ccd_mode, n, d_mode); GROW(b_ccd_bmode, dw.n_bodies, d_bmode);
            std::vector<uint32_t> bmode(dw.n_bodies, 0u);
            for (uint32_t i = 0; i < n; ++i) if (l->mode[i] == AVN_SWEEP_NON_LINEAR) bmode[l->body[i]] = 1u;
            HIPCHK(hipMemcpy(d_mode, l->mode, (size_t)n * 4, hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(d_bmode, bmode.data(), (size_t)dw.n_bodies * 4, hipMemcpyHostToDevice));
        }
        HIPCHK(hipMemset(b_ccd_sums.p, 0, b_ccd_sums.cap));   // the one-launch scan's state: zero once, self-cleaning afterwards (avn_scan.h)
        HIPCHK(hipMemcpy(d_body, l->body, (size_t)n * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_incl, incl.data(), (size_t)n * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_lin2, lin2.data(), (size_t)n * sizeof(T), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_ang2, ang2.data(), (size_t)n * sizeof(T), hipMemcpyHostToDevice));
        c.n = n; c.body = d_body; c.include_dynamic = d_incl; c.lin2 = d_lin2; c.ang2 = d_ang2; c.mode = d_mode; c.body_mode = d_bmode;
        ccd = c;
        ccd_ran = false; ccd_tables_dirty = true;
        if (!ev_ccd) HIPCHK(hipEventCreateWithFlags(&ev_ccd, EV_FLAGS));
        return AVN_OK;
    }

    // between the substep loop (every island stream joined) and the restitution pass, on the world's stream
    avn_status ccd_pass() {
        if (ccd_tables_dirty) {
            GROW(b_ccd_entry, std::max<size_t>(bp.n_colliders, 1), ccd.entry);
            launch_ccd_tables<T>(dw, bp, ccd, stream); launches += 4;
            ccd_tables_dirty = false;
        }
        // a row with two CCD sides yields two candidates
        if (2 * (size_t)ct.cap > ccd.cand_cap || !ccd.cand) {
            const size_t cap = std::max<size_t>(2 * (size_t)ct.cap, 64);
            GROW(b_ccd_cand, cap, ccd.cand); GROW(b_ccd_cand_t, cap, ccd.cand_t);
            ccd.cand_cap = (uint32_t)std::min<size_t>(cap, 0xFFFFFFFFu);
        }
        launches += launch_ccd_pass<T>(dw, bp, ct, pg, ccd, params, pgm_next_id, stream, ccd_caps_on && cap_count != 0);   // (a world without a capsule, or with the switch off, launches what it always has)
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ev_ccd, stream));
        ccd_stamped = true; ccd_ran = true;
        return AVN_OK;
    }

    avn_status swept_ccd_results_get(avn_swept_ccd_results_out* out) override {
        if (!out) { error = "swept_ccd_results_get: null argument"; return AVN_ERR_BAD_ARG; }
        out->count = ccd_ran ? ccd.n : 0u;
        if (!out->count) return AVN_OK;
        if (out->results && out->capacity < out->count) { error = "swept_ccd_results_get: more entries than capacity"; return AVN_ERR_CAPACITY; }
        HIPCHK(hipStreamSynchronize(stream));
        if (out->results) HIPCHK(hipMemcpy(out->results, ccd.rec, (size_t)ccd.n * sizeof(SweptCcdResult<T>), hipMemcpyDeviceToHost));
        return AVN_OK;
    }

    avn_status swept_ccd_non_linear_set(uint32_t enabled) override {
        if (!enabled && ccd.n && ccd.mode) { error = "swept_ccd_non_linear_set: the list in force holds an AVN_SWEEP_NON_LINEAR entry; avn_swept_ccd_upload another list first"; return AVN_ERR_STATE; }
        ccd_nl_on = enabled != 0;
        return AVN_OK;
    }

    avn_status swept_ccd_capsules_set(uint32_t enabled) override { ccd_caps_on = enabled != 0; return AVN_OK; }   // (read per pass: nothing to strand)

    avn_status swept_ccd_stats_get(avn_swept_ccd_stats* out) override {
        if (!out || out->struct_size != sizeof(avn_swept_ccd_stats)) { error = "swept_ccd_stats_get: null argument or struct_size"; return AVN_ERR_BAD_ARG; }
        out->nonlinear_tested = out->rounds_max = out->exhausted = 0u;
        if (!ccd_ran || !ccd.n) return AVN_OK;
        HIPCHK(hipStreamSynchronize(stream));
        uint32_t ctr[4];
        HIPCHK(hipMemcpy(ctr, ccd.ctr, sizeof(ctr), hipMemcpyDeviceToHost));
        out->nonlinear_tested = ctr[CCD_CTR_NL_TESTED]; out->rounds_max = ctr[CCD_CTR_ROUNDS_MAX]; out->exhausted = ctr[CCD_CTR_EXHAUSTED];
        return AVN_OK;
    }
