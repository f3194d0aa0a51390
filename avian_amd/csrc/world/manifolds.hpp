// world/manifolds.hpp -- fragment of the body of `template <class T> struct World` (avn_world.hip includes it inside the class):
// host-uploaded manifolds, the warm start's incidence, island blocks, impulse / constraint read-back.

    // ---- manifolds ---------------------------------------------------------------------------------------
    // Level compaction (k_levels.hip): the upload regroups colours 0..22 into the levels of the per-body order the colouring
    // fixes.  The device arrays and color_offsets are then level-major; lvl_perm maps an upload position to its device position, and every
    // reader of manifold-indexed data behind the ABI goes through it (the unpack kernels) or sees host copies already translated (h_m_body1/2).
    DevBuf b_lvl_perm;
    bool lvl_active = false;                 // the manifolds on the device are level-major (lvl_perm valid); cleared by every set_color_offsets
    bool lvl_level2 = false;                 // the level-2 / per-colour API was used on this world: ranks must agree on the colours -- never compact again
#ifdef AVN_MEASURE
    bool lvl_enabled = avn_env("AVN_NO_LEVEL_COMPACTION") == nullptr;   // (A/B, and the tests' second reference: colour launches as before)
#else
    static constexpr bool lvl_enabled = true;
#endif
    uint32_t lvl_uploaded_offsets[AVN_GRAPH_COLOR_COUNT + 1] = {0};     // the colour offsets of the last manifolds_upload, as the host sent them
    Pinned pin_lvl;                          // the result words of an upload's compaction (LVL_RES_*), read back with the synchronisation the upload ends with
    hipEvent_t ev_lvl_go = nullptr, ev_lvl_done = nullptr;   // body1 / body2 are on the device -> the level kernels on the second stream -> k_pack_manifolds
    avn_level_compaction_stats lvl_stats{};
    const uint32_t* lvl_perm() const { return lvl_active ? b_lvl_perm.as<uint32_t>() : nullptr; }
    void lvl_note(uint32_t state, uint32_t why, const uint32_t* uploaded, const uint32_t* now, uint32_t max_degree, uint32_t moved) {
        lvl_stats = avn_level_compaction_stats{};
        lvl_stats.state = state; lvl_stats.why_off = why; lvl_stats.max_degree = max_degree; lvl_stats.moved = moved;
        for (int c = 0; c < AVN_COLOR_OVERFLOW_INDEX; ++c) {
            lvl_stats.colours += uploaded[c + 1] > uploaded[c] ? 1u : 0u;
            lvl_stats.sizes[c] = now[c + 1] - now[c];
            lvl_stats.levels += lvl_stats.sizes[c] ? 1u : 0u;
        }
    }
    avn_status level_compaction_stats_get(avn_level_compaction_stats* out) override {
        if (!out || out->struct_size != sizeof(avn_level_compaction_stats)) { error = "level_compaction_stats_get: null argument or struct_size"; return AVN_ERR_BAD_ARG; }
        *out = lvl_stats;
        if (pipe_on || use_handles) {   // the lists are the bookkeeping's, not an upload's: answered from the ranges as they are, nothing is stored
            *out = avn_level_compaction_stats{};
            out->why_off = AVN_LEVELS_WHY_CLOSED_LOOP;
            for (int c = 0; c < AVN_COLOR_OVERFLOW_INDEX; ++c) { out->sizes[c] = color_offsets[c + 1] - color_offsets[c]; out->colours += out->sizes[c] ? 1u : 0u; }
            out->levels = out->colours;
        }
        out->overflow_first = color_offsets[AVN_COLOR_OVERFLOW_INDEX]; out->overflow_count = color_offsets[AVN_COLOR_OVERFLOW_INDEX + 1] - color_offsets[AVN_COLOR_OVERFLOW_INDEX];
        out->struct_size = (uint32_t)sizeof(avn_level_compaction_stats);
        return AVN_OK;
    }
    // The level-2 / per-colour API (halo plan, overflow levels, joint slot, run_color_pass, comm_init) addresses the host's COLOURS: from its first
    // use on the world stays in colour order, and a set that was compacted before is put back (every manifold-indexed array, upload order).
    avn_status level_uncompact() {
        { const avn_status sm = materialize_impulses(); if (sm != AVN_OK) return sm; }   // (mp_w moves below; the level-2 calls behind this one run passes of their own on c_pd)
        lvl_level2 = true;
        if (!lvl_active) {
            if (lvl_stats.state != AVN_LEVELS_OFF) lvl_note(AVN_LEVELS_OFF, AVN_LEVELS_WHY_LEVEL2, color_offsets, color_offsets, 0u, 0u);   // (an early-out set is in colour order already)
            return AVN_OK;
        }
        const uint32_t M = dw.n_manifolds;
        const uint32_t* perm = b_lvl_perm.as<uint32_t>();
        HIPCHK(hipStreamSynchronize(stream));
        if (stream_bp) HIPCHK(hipStreamSynchronize(stream_bp));
        DevBuf tmp;
        ALLOC(tmp.ensure((size_t)M * sizeof(V)));
        auto put_back = [&](void* arr, size_t elem, uint32_t planes) -> hipError_t {
            for (uint32_t k = 0; k < planes; ++k) {
                char* a = (char*)arr + (size_t)k * dw.m_stride * elem;
                if (!launch_level_unpermute(tmp.p, a, elem, perm, M, stream)) return hipErrorInvalidValue;
                hipError_t e = hipMemcpyAsync(a, tmp.p, (size_t)M * elem, hipMemcpyDeviceToDevice, stream);
                if (e != hipSuccess) return e;
            }
            return hipSuccess;
        };
        HIPCHK(put_back(dw.m_bodies, sizeof(int2), 1)); HIPCHK(put_back(dw.m_n, sizeof(V), 1)); HIPCHK(put_back(dw.m_tv, sizeof(V), 1)); HIPCHK(put_back(dw.m_meta, 4, 1));
        HIPCHK(put_back(dw.mp_a1, sizeof(V), 4)); HIPCHK(put_back(dw.mp_a2, sizeof(V), 4)); HIPCHK(put_back(dw.mp_w, sizeof(V), 4));
        HIPCHK(put_back(dw.c_h1, sizeof(V), 1)); HIPCHK(put_back(dw.c_pa, sizeof(V), 4)); HIPCHK(put_back(dw.c_pb, sizeof(V), 4)); HIPCHK(put_back(dw.c_pc, sizeof(V), 4));
        HIPCHK(put_back(dw.c_pd, sizeof(V), 4)); HIPCHK(put_back(dw.c_reldom, sizeof(int16_t), 1));
        HIPCHK(hipMemcpyAsync(dw.color_offsets, lvl_uploaded_offsets, sizeof lvl_uploaded_offsets, hipMemcpyHostToDevice, stream));
        if (h_m_body1.size() == M && lvl_host_translated) {   // the host copies back into upload order as well
            std::vector<uint32_t> hp(M);
            HIPCHK(hipMemcpyAsync(hp.data(), perm, (size_t)M * 4, hipMemcpyDeviceToHost, stream));
            HIPCHK(hipStreamSynchronize(stream));
            std::vector<int32_t> a(M), b(M);
            for (uint32_t i = 0; i < M; ++i) { a[i] = h_m_body1[hp[i]]; b[i] = h_m_body2[hp[i]]; }
            h_m_body1.swap(a); h_m_body2.swap(b);
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(stream));
        set_color_offsets(lvl_uploaded_offsets);   // (clears lvl_active; the captured ranges differ: re-capture)
        lvl_note(AVN_LEVELS_OFF, AVN_LEVELS_WHY_LEVEL2, color_offsets, color_offsets, 0u, 0u);
        graph_valid = false; incidence_dirty = true;
        return AVN_OK;
    }
    bool lvl_host_translated = false;   // h_m_body1 / h_m_body2 are in device order (sets small enough for the island blocks, whose entry lists are host-built)
    avn_status manifolds_upload(const avn_manifolds* m) override {
        if (!have_bodies) { error = "manifolds_upload before bodies_upload"; return AVN_ERR_STATE; }
        if (!m || !m->color_offsets || (m->count && (!m->body1 || !m->body2 || !m->normal || !m->friction || !m->restitution || !m->point_count ||
                                                    !m->anchor1 || !m->anchor2 || !m->penetration || !m->normal_speed))) {
            error = "manifolds_upload: null array"; return AVN_ERR_BAD_ARG;
        }
        uint32_t M = m->count;
        if (m->color_offsets[0] != 0 || m->color_offsets[AVN_GRAPH_COLOR_COUNT] != M) { error = "manifolds_upload: bad color_offsets"; return AVN_ERR_BAD_ARG; }
        for (int c = 0; c < AVN_GRAPH_COLOR_COUNT; ++c)
            if (m->color_offsets[c] > m->color_offsets[c + 1]) { error = "manifolds_upload: color_offsets not monotone"; return AVN_ERR_BAD_ARG; }
        { const avn_status sm = materialize_impulses(); if (sm != AVN_OK) return sm; }   // (with the OLD count: an upload that is rejected below leaves mp_w as a step with its store would have)
        if (use_handles) graph_valid = false;
        use_handles = false;  // the manifolds come from the host again
        lvl_active = false;   // (the permutation describes the previous set: an upload that fails half way must not leave it in force)
        avn_status st0 = ensure_manifold_capacity(M);
        if (st0 != AVN_OK) return st0;
        if (dw.n_manifolds != M) graph_valid = false;
        dw.n_manifolds = M;
        // level compaction: wanted unless the world's lists are not host manifolds, it is a level-2 rank, or there is nothing to regroup
        uint32_t populated = 0;
        for (int c = 0; c < AVN_COLOR_OVERFLOW_INDEX; ++c) populated += m->color_offsets[c + 1] > m->color_offsets[c] ? 1u : 0u;
        const uint32_t why_off = !lvl_enabled ? AVN_LEVELS_WHY_SWITCH : (pipe_on || pipe_dev) ? AVN_LEVELS_WHY_CLOSED_LOOP : (lvl_level2 || halo_on) ? AVN_LEVELS_WHY_LEVEL2
                                 : populated == 0 ? AVN_LEVELS_WHY_EMPTY : AVN_LEVELS_WHY_NONE;
        const bool lvl_try = why_off == AVN_LEVELS_WHY_NONE && populated >= 2;   // (one colour: one launch either way -- the early out, known without a reduction)
        std::memcpy(lvl_uploaded_offsets, m->color_offsets, sizeof lvl_uploaded_offsets);
        lvl_host_translated = false;
        // (one set_color_offsets per upload, with the offsets the solver will run: a host that re-sends a settled pile's manifolds every step keeps its captured graph)
        if (!lvl_try) {
            set_color_offsets(m->color_offsets);
            lvl_note(why_off == AVN_LEVELS_WHY_NONE ? AVN_LEVELS_EARLY_OUT : AVN_LEVELS_OFF, why_off, m->color_offsets, m->color_offsets, 0u, 0u);
        }
        ManifoldStage<T> s;
        std::memset(&s, 0, sizeof s);
        StagePlan plan(*this);
        // The level kernels need body1 / body2 only, the first two of the fourteen arrays: they run on the second stream behind an event recorded after those two copies,
        // under the remaining copies and the host's pass below; k_pack_manifolds waits for their event, and the early out is decided on the device (k_level_scatter).  No
        // host synchronisation but the one the upload ends with.
        uint32_t *lvl_zeroed = nullptr, *lvl_hist = nullptr; uint8_t* lvl_level = nullptr;
        const uint32_t nb_ = dw.n_bodies;
        LevelOffsets lo;
        std::memcpy(lo.o, lvl_uploaded_offsets, sizeof lo.o);
        if (lvl_try) {
            plan.scratch((size_t)level_zeroed_words(nb_, M), &lvl_zeroed); plan.scratch((size_t)AVN_COLOR_OVERFLOW_INDEX * level_tiles(M), &lvl_hist); plan.scratch((size_t)M, &lvl_level);
            ALLOC(b_lvl_perm.ensure((size_t)M * 4));
            ALLOC(pin_lvl.ensure(LVL_RES_WORDS * 4));
            if (!ev_lvl_go) { HIPCHK(hipEventCreateWithFlags(&ev_lvl_go, hipEventDisableTiming | EV_FLAGS)); HIPCHK(hipEventCreateWithFlags(&ev_lvl_done, hipEventDisableTiming | EV_FLAGS)); }
        }
        SIN(body1, m->body1, M); SIN(body2, m->body2, M);
        if (lvl_try) {
            plan.hook_after = plan.l.n - 1;
            // (the hook only marks the place in the stream: the chain's two dozen launches are enqueued once every copy is on its way -- enqueued here they held the
            //  remaining copies back by their host time, 0.1 ms of a 1 ms upload)
            plan.hook = [&]() -> avn_status { HIPCHK(hipEventRecord(ev_lvl_go, stream)); return AVN_OK; };
        }
        SIN(normal, m->normal, 3 * (size_t)M);
        SIN(friction, m->friction, M); SIN(restitution, m->restitution, M); SIN(tangent_velocity, m->tangent_velocity, 3 * (size_t)M);
        SIN(point_count, m->point_count, M); SIN(manifold_flags, m->manifold_flags, M);
        SIN(anchor1, m->anchor1, 12 * (size_t)M); SIN(anchor2, m->anchor2, 12 * (size_t)M);
        SIN(penetration, m->penetration, 4 * (size_t)M); SIN(normal_speed, m->normal_speed, 4 * (size_t)M);
        SIN(warm_n, m->warm_start_normal_impulse, 4 * (size_t)M); SIN(warm_t, m->warm_start_tangent_impulse, 8 * (size_t)M);
        COMMIT(plan);
        HIPCHK(hipMemcpyAsync(dw.color_offsets, lvl_uploaded_offsets, sizeof lvl_uploaded_offsets, hipMemcpyHostToDevice, stream));
        uint32_t* lvl_res = lvl_try ? lvl_zeroed + 2 * (size_t)nb_ : nullptr;
        if (lvl_try) {
            HIPCHK(hipStreamWaitEvent(stream_bp, ev_lvl_go, 0));
            HIPCHK(hipMemsetAsync(lvl_zeroed, 0, (size_t)level_zeroed_words(nb_, M) * 4, stream_bp));
            launches += launch_level_build(s.body1, s.body2, nb_, lo, populated, lvl_zeroed, lvl_level, lvl_hist, b_lvl_perm.as<uint32_t>(), stream_bp);
            HIPCHK(hipGetLastError());
            HIPCHK(hipEventRecord(ev_lvl_done, stream_bp));
            HIPCHK(hipStreamWaitEvent(stream, ev_lvl_done, 0));
            HIPCHK(hipMemcpyAsync(dw.color_offsets, lvl_res, AVN_COLOR_OVERFLOW_INDEX * 4, hipMemcpyDeviceToDevice, stream));   // (the ranges of colours 0..22 as the device decided them)
            HIPCHK(hipMemcpyAsync(pin_lvl.p, lvl_res, LVL_RES_WORDS * 4, hipMemcpyDeviceToHost, stream));
        }
        launch_pack_manifolds<T>(dw, s, lvl_try ? b_lvl_perm.as<uint32_t>() : nullptr, stream);
        HIPCHK(hipGetLastError());
        // (while the copies run) one pass over the host arrays: range checks, "any restitution", and the host copy of the ContactPair bodies (incidence CSR source)
        {
            const uint32_t nb = dw.n_bodies;
            const T* rest = (const T*)m->restitution;
            h_m_body1.resize(M); h_m_body2.resize(M);
            bool bad_body = false, bad_pc = false, any_r = false;
            for (uint32_t i = 0; i < M; ++i) {
                const int32_t a = m->body1[i], b = m->body2[i];
                bad_body |= (uint32_t)a >= nb || (uint32_t)b >= nb;   // (negative indices wrap above nb)
                bad_pc |= m->point_count[i] > AVN_MAX_MANIFOLD_POINTS;
                any_r |= !(rest[i] == T(0));
                h_m_body1[i] = a; h_m_body2[i] = b;
            }
            any_restitution = any_r;
            if (bad_body || bad_pc) {   // nothing of a rejected upload may be solved: the world is left without manifolds
                HIPCHK(hipStreamSynchronize(stream));
                uint32_t zero[AVN_GRAPH_COLOR_COUNT + 1] = {0};
                dw.n_manifolds = 0; h_m_body1.clear(); h_m_body2.clear();
                set_color_offsets(zero);
                lvl_note(AVN_LEVELS_OFF, AVN_LEVELS_WHY_EMPTY, zero, zero, 0u, 0u);
                HIPCHK(hipMemcpyAsync(dw.color_offsets, zero, sizeof zero, hipMemcpyHostToDevice, stream));
                HIPCHK(hipStreamSynchronize(stream));
                graph_valid = false; incidence_dirty = true;
                error = bad_body ? "manifolds_upload: body index out of range" : "manifolds_upload: point_count > 4";
                return AVN_ERR_BAD_ARG;
            }
        }
        if (lvl_try) {
            std::vector<uint32_t> hp;
            if (M <= island_max_manifolds) {   // (island_candidate's bound on the set, whatever bodies are uploaded later: the island-block builder reads the host copies by device position)
                hp.resize(M);
                HIPCHK(hipMemcpyAsync(hp.data(), b_lvl_perm.p, (size_t)M * 4, hipMemcpyDeviceToHost, stream));
            }
            HIPCHK(hipStreamSynchronize(stream));   // the synchronisation every upload ends with
            const uint32_t* r = (const uint32_t*)pin_lvl.p;
            uint32_t now[AVN_GRAPH_COLOR_COUNT + 1];
            std::memcpy(now, lvl_uploaded_offsets, sizeof now);
            std::memcpy(now, r, AVN_COLOR_OVERFLOW_INDEX * 4);
            const uint32_t max_degree = r[LVL_RES_MAX_DEGREE], moved = r[LVL_RES_MOVED];
            const bool early = max_degree == populated;   // (k_level_scatter's own test: it left the identity and the uploaded offsets)
            set_color_offsets(now);
            lvl_active = !early;
            lvl_note(early ? AVN_LEVELS_EARLY_OUT : AVN_LEVELS_COMPACTED, AVN_LEVELS_WHY_NONE, lvl_uploaded_offsets, now, max_degree, moved);
            lvl_host_translated = !early && !hp.empty();
            if (lvl_host_translated) for (uint32_t i = 0; i < M; ++i) { h_m_body1[hp[i]] = m->body1[i]; h_m_body2[hp[i]] = m->body2[i]; }
        }
        incidence_dirty = true;
        HIPCHK(hipStreamSynchronize(stream));
        return AVN_OK;
    }
    // Incidence CSR of the body-centric warm start: per body that has a SolverBody, its (manifold, side) entries in SOLVE
    // order = overflow colour first, then colours 0..22 (reference plugin.rs:461-470), list order inside a colour.
    // Incidence of the body-centric warm start.  Colours 0..22: the slot table is (re)built ON THE DEVICE from the manifold arrays
    // (launch_build_incidence_slots, run after the manifolds are in place).  Host part: only the overflow colour -- its
    // per-body entry lists (CSR, list order) and its level schedule.
    bool slots_dirty = true;
    bool ovf_csr_dirty = false;
    avn_status rebuild_incidence() {
        if (!incidence_dirty) return AVN_OK;
        groups_dirty = true;   // bodies, manifolds or their mode changed: the island streams' grouping follows
        if (pipe_dev) { ovf_csr_dirty = true; return rebuild_incidence_device(); }
        uint32_t N = dw.n_bodies, M = dw.n_manifolds;
        if (M == 0) { incidence_dirty = false; island_mode = false; islands_dirty = false; return AVN_OK; }
        if (h_body_has_sb.size() != N || h_m_body1.size() != M) { error = "incidence: bodies / manifolds out of sync"; return AVN_ERR_STATE; }
        HIPCHK(hipStreamSynchronize(stream));
        {   // slot table storage: 23 colour planes of cap_bodies entries
            bool moved = false;
            ALLOC(b_inc_slot.ensure((size_t)AVN_COLOR_OVERFLOW_INDEX * cap_bodies * sizeof(uint32_t), &moved));
            if (moved || dw.inc_stride != cap_bodies) graph_valid = false;
            dw.inc_slot = b_inc_slot.as<uint32_t>();
            dw.inc_stride = cap_bodies;
            slots_dirty = true;
        }
        const uint32_t o0 = color_offsets[AVN_COLOR_OVERFLOW_INDEX], o1 = color_offsets[AVN_COLOR_OVERFLOW_INDEX + 1];
        std::vector<uint32_t>& off = inc_off_h; std::vector<uint32_t>& cursor = inc_cursor_h; std::vector<uint32_t>& ent = inc_ent_h;
        off.assign((size_t)N + 1, 0u);
        for (uint32_t m = o0; m < o1; ++m) {
            if (h_body_has_sb[h_m_body1[m]]) ++off[(size_t)h_m_body1[m] + 1];
            if (h_body_has_sb[h_m_body2[m]]) ++off[(size_t)h_m_body2[m] + 1];
        }
        for (uint32_t i = 0; i < N; ++i) off[i + 1] += off[i];
        cursor.assign(off.begin(), off.end() - 1);
        ent.resize(off[N]);
        for (uint32_t m = o0; m < o1; ++m) {
            uint32_t a = (uint32_t)h_m_body1[m], b = (uint32_t)h_m_body2[m];
            if (h_body_has_sb[a]) ent[cursor[a]++] = m;
            if (h_body_has_sb[b]) ent[cursor[b]++] = m | 0x80000000u;
        }
        bool moved = false;
        ALLOC(b_inc_off.ensure(((size_t)N + 1) * 4, &moved));
        ALLOC(b_inc_ent.ensure(std::max<size_t>(ent.size(), 1) * sizeof(uint32_t), &moved));
        if (moved || !dw.inc_off) graph_valid = false;
        dw.inc_off = b_inc_off.as<uint32_t>();
        dw.inc_ent = b_inc_ent.as<uint32_t>();
        if (o1 > o0 || overflow_csr_nonzero) {   // an all-zero offset array stays valid while the overflow colour is empty
            HIPCHK(hipMemcpyAsync(b_inc_off.p, off.data(), off.size() * 4, hipMemcpyHostToDevice, stream));
            if (!ent.empty()) HIPCHK(hipMemcpyAsync(b_inc_ent.p, ent.data(), ent.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
            HIPCHK(hipStreamSynchronize(stream));
            overflow_csr_nonzero = o1 > o0;
        } else if (moved || overflow_csr_bodies != N) {
            HIPCHK(hipMemsetAsync(b_inc_off.p, 0, ((size_t)N + 1) * 4, stream));
        }
        overflow_csr_bodies = N;
        {   // level schedule of the overflow colour (k_overflow_pass): keys = the bodies a manifold can modify
            std::vector<uint32_t> ms(o1 - o0);
            std::vector<int32_t> k1(o1 - o0), k2(o1 - o0);
            for (uint32_t m = o0; m < o1; ++m) {
                ms[m - o0] = m;
                k1[m - o0] = h_body_has_sb[h_m_body1[m]] ? h_m_body1[m] : -1;
                k2[m - o0] = h_body_has_sb[h_m_body2[m]] ? h_m_body2[m] : -1;
            }
            uint32_t before = sched_overflow.n_components;
            const bool levels_before = sched_overflow.gorder.size() > overflow_level_threshold;   // (the form contact_pass picks: one device-wide launch per LEVEL, sizes captured)
            const std::vector<uint32_t> glevels_before = levels_before ? sched_overflow.glevel_offsets : std::vector<uint32_t>();
            sched_overflow.build(ms, k1, k2, N, ms.size() > overflow_level_threshold);
            void* p0 = sched_overflow.d_order.p; void* p1 = sched_overflow.d_level_offsets.p; void* p2 = sched_overflow.d_comp_level_begin.p; void* p3 = sched_overflow.d_gorder.p;
            avn_status st;
            if ((st = upload_u32(sched_overflow.d_comp_level_begin, sched_overflow.comp_level_begin)) != AVN_OK) return st;
            if ((st = upload_u32(sched_overflow.d_level_offsets, sched_overflow.level_offsets)) != AVN_OK) return st;
            if ((st = upload_u32(sched_overflow.d_order, sched_overflow.order)) != AVN_OK) return st;
            if ((st = upload_u32(sched_overflow.d_gorder, sched_overflow.gorder)) != AVN_OK) return st;
            HIPCHK(hipStreamSynchronize(stream));
            // What the substep graph captured of the overflow colour: per-component form (k_overflow_pass) -- the grid (n_components) and the three pointers, checked
            // below; the arrays are read at replay.  Per-level form -- every level's (first, count) as launch parameters: re-capture when they differ.  (Until round 6
            // ANY non-empty overflow colour invalidated the graph with every upload: a host that re-sends a settled pile's manifolds every step -- HostNarrowPhase mode --
            // paid a capture + instantiate per step for a schedule that had not changed.)
            const bool levels_now = sched_overflow.gorder.size() > overflow_level_threshold;
            if (levels_now != levels_before || (levels_now && glevels_before != sched_overflow.glevel_offsets)) graph_valid = false;
            if (before != sched_overflow.n_components || p0 != sched_overflow.d_order.p || p1 != sched_overflow.d_level_offsets.p || p2 != sched_overflow.d_comp_level_begin.p || p3 != sched_overflow.d_gorder.p) graph_valid = false;
        }
        islands_dirty = true;   // rebuilt by solver_front AFTER the prepare kernels are enqueued (host work overlaps them)
        incidence_dirty = false;
        return AVN_OK;
    }
    // Island blocks (k_island_substeps).  Islands = connected components of the bodies that have a SolverBody under "share a
    // manifold" (a body without one -- static, sleeping, disabled -- is never written by the solver and joins nothing;
    // kinematic bodies DO have a SolverBody that the solver reads and re-writes, so they merge like dynamic ones).  Eligible
    // when f32, no joints, few enough manifolds for the colour launches to be latency-bound and every island fits a block.
    // (... and few enough BODIES: the block builder is host code that touches every body with a SolverBody, and the one launch stages all of
    //  them in LDS -- at cfg4's 10^6 free bodies around 2 k manifolds the attempt cost 5 ms of host time per step, found by the stepped cfg4 timing)
    size_t island_max_bodies_total = 65536;
    bool island_candidate(size_t M) const { return sizeof(T) == 4 && island_enabled && M != 0 && M <= island_max_manifolds && dw.n_bodies <= island_max_bodies_total; }
    avn_status rebuild_island_blocks() {
        island_mode = false;
        const uint32_t N = dw.n_bodies, M = dw.n_manifolds;
        if (!island_candidate(M) || dw.n_joints) return AVN_OK;
        auto has_sb = [&](int32_t b) { return b >= 0 && (uint32_t)b < N && h_body_has_sb[(uint32_t)b]; };
        std::vector<uint32_t>& parent = isl_parent;
        parent.resize(N);
        bool labelled = false;
        static const bool host_labels = avn_env("AVN_ISLAND_LABELS_HOST") != nullptr;   // A/B: the host union-find below
        if (pipe_dev && slp_on && !host_labels) {
            // sleeping on: the persistent islands ARE a grouping of the awake bodies no manifold crosses (an island pending its split is merely
            // coarser than necessary) -- taken straight from the manager: no labelling kernel, no read-back, no synchronisation
            std::vector<uint32_t>& rep = isl_roots;
            rep.assign((size_t)isl.island_key_bound(), 0xFFFFFFFFu);
            for (uint32_t i = 0; i < N; ++i) {
                parent[i] = i;
                if (!h_body_has_sb[i] || !isl.body_has_node(i)) continue;
                const uint32_t k = isl.island_of(i);
                if (rep[k] == 0xFFFFFFFFu) rep[k] = i;
                parent[i] = rep[k];
            }
            isl_labels_step_valid = false;
            labelled = true;
        } else if (pipe_dev && !host_labels) {
            // device closed loop: the manifolds' bodies are on the device already -- label the islands there (k_islands.hip: lock-free
            // union-find, root = lowest body index, only bodies with a SolverBody connect) and fetch 4 bytes per body; parent[] then holds
            // roots directly
            avn_status st = island_buffers();
            if (st != AVN_OK) return st;
            HIPCHK(hipMemsetAsync(b_isl_ctr.p, 0, 64, stream));
            bool reuse = false;
            if (isl_labels_step_valid && isl_roots.size() == N) {
                // last step's labels, checked against this step's manifolds on the device: one small kernel and a 4-byte read-back instead of
                // the union-find (100 us at 13 k manifolds: deep trees under "root = lowest index") and the read-back of every label
                launch_islands_validate<T>(dw, b_isl_blk_label.as<uint32_t>(), b_isl_ctr.as<uint32_t>() + 8, stream, 1u);
                ++launches;
                uint32_t invalid = 1;
                HIPCHK(hipMemcpyAsync(&invalid, b_isl_ctr.as<uint32_t>() + 8, 4, hipMemcpyDeviceToHost, stream));
                HIPCHK(hipStreamSynchronize(stream));
                reuse = invalid == 0;
            }
            if (reuse) parent = isl_roots;
            else {
                launch_islands<T>(dw, b_isl_parent.as<uint32_t>(), b_isl_blk_label.as<uint32_t>(), b_isl_ctr.as<uint32_t>(), stream, 1u);
                launches += 3;
                HIPCHK(hipMemcpyAsync(parent.data(), b_isl_blk_label.p, (size_t)N * 4, hipMemcpyDeviceToHost, stream));
                HIPCHK(hipStreamSynchronize(stream));
                isl_roots = parent;   // (as the device holds them: 0xFFFFFFFF for a body that was no island node)
                isl_labels_step_valid = true;
            }
            for (uint32_t i = 0; i < N; ++i) if (parent[i] == 0xFFFFFFFFu || !h_body_has_sb[i]) parent[i] = i;   // (bodies without a SolverBody: never asked)
            labelled = true;
        } else for (uint32_t i = 0; i < N; ++i) parent[i] = i;
        auto find = [&](uint32_t x) { while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; } return x; };
        for (uint32_t m = 0; m < M && !labelled; ++m) {
            int32_t a = h_m_body1[m], b = h_m_body2[m];
            if (has_sb(a) && has_sb(b)) { uint32_t ra = find((uint32_t)a), rb = find((uint32_t)b); if (ra != rb) parent[std::max(ra, rb)] = std::min(ra, rb); }
        }
        // islands numbered by their lowest body (the root: unions keep the smaller index on top), bodies inside in index order
        std::vector<uint32_t>& island_of = isl_island_of; std::vector<uint32_t>& count = isl_count;
        island_of.assign(N, 0xFFFFFFFFu);
        std::vector<uint32_t>& root_island = isl_root_island;
        root_island.assign(N, 0xFFFFFFFFu);
        count.clear();
        for (uint32_t i = 0; i < N; ++i) {
            if (!h_body_has_sb[i]) continue;
            uint32_t r = find(i);
            // (with REUSED labels the root -- the lowest index of the component when it was labelled -- may have lost its SolverBody since: it
            //  then only lends its index to the group, so the root's island is kept apart from island_of, which lists MEMBERS)
            if (root_island[r] == 0xFFFFFFFFu) { root_island[r] = (uint32_t)count.size(); count.push_back(0u); }
            island_of[i] = root_island[r];   // islands are numbered by their first member with a SolverBody, bodies inside in index order
            if (++count[island_of[i]] > ISLAND_MAX_BODIES) return AVN_OK;   // an island too big for one workgroup's LDS: device-wide path
        }
        const uint32_t n_islands = (uint32_t)count.size();
        if (!n_islands) return AVN_OK;
        // manifolds per island (a manifold belongs to the island of its body that has a SolverBody)
        std::vector<uint32_t>& mcount = isl_mcount;
        mcount.assign(n_islands, 0u);
        for (uint32_t m = 0; m < M; ++m) {
            int32_t a = h_m_body1[m], b = h_m_body2[m];
            if (has_sb(a)) ++mcount[island_of[(uint32_t)a]]; else if (has_sb(b)) ++mcount[island_of[(uint32_t)b]]; else ++mcount[0];
        }
        // blocks = runs of consecutive islands of at most island_pack_bodies bodies (one island may exceed that, up to the LDS cap);
        // a run is also closed when its bodies + constraint records would no longer fit the LDS staging of the kernel's CACHE variant
        std::vector<uint32_t>& block_of = isl_block_of_island; std::vector<uint32_t>& body_off = isl_body_off;
        block_of.resize(n_islands);
        body_off.assign(1, 0u);
        std::vector<uint32_t>& cursor = isl_cursor;   // per island: next LDS slot
        cursor.resize(n_islands);
        // pack target: enough blocks to cover the 256 CUs before blocks grow (a block's pass time is flat up to ~256 manifolds per colour)
        uint32_t n_sb = 0;
        for (uint32_t k = 0; k < n_islands; ++k) n_sb += count[k];
        const uint32_t pack = std::min<uint32_t>(island_pack_bodies, std::max<uint32_t>(64u, (n_sb + 255u) / 256u));
        uint32_t in_block = 0, m_in_block = 0, max_bodies = 0, max_manifolds = 0;
        auto close_block = [&]() { max_bodies = std::max(max_bodies, in_block); max_manifolds = std::max(max_manifolds, m_in_block); body_off.push_back(body_off.back() + in_block); in_block = 0; m_in_block = 0; };
        for (uint32_t k = 0; k < n_islands; ++k) {
            if (in_block && (in_block + count[k] > pack || 6u * (in_block + count[k]) + 20u * (m_in_block + mcount[k]) > ISLAND_LDS_VEC4)) close_block();
            block_of[k] = (uint32_t)body_off.size() - 1;
            cursor[k] = in_block;
            in_block += count[k];
            m_in_block += mcount[k];
        }
        close_block();
        // the LDS layout is the same for every block (sized by the largest body and manifold counts)
        const uint32_t lm_pad = (max_manifolds + 1u) & ~1u;   // (the entry list behind the records is uint2: keep it 16-byte aligned)
        const bool cache_records = island_cache_records && 6u * max_bodies + 20u * lm_pad <= ISLAND_LDS_VEC4;
        const uint32_t n_blocks = (uint32_t)body_off.size() - 1;
        std::vector<uint32_t>& slot = isl_slot; std::vector<uint32_t>& bodies = isl_bodies;
        slot.assign(N, 0u);
        bodies.resize(body_off.back());
        for (uint32_t i = 0; i < N; ++i) {
            uint32_t k = island_of[i];
            if (k == 0xFFFFFFFFu) continue;
            slot[i] = cursor[k]++;
            bodies[body_off[block_of[k]] + slot[i]] = i;
        }
        // entries: counting sort of the manifolds by (block, colour slot), ascending manifold index inside (= list order: the
        // overflow colour's serial order); colour slot 0 = overflow (solved first), 1 + c = colour c
        std::vector<uint32_t>& col_off = isl_col_off; std::vector<uint32_t>& ent = isl_ent;
        col_off.assign((size_t)n_blocks * AVN_GRAPH_COLOR_COUNT + 1, 0u);
        auto key_of = [&](uint32_t m, uint32_t c) -> size_t {
            int32_t a = h_m_body1[m], b = h_m_body2[m];
            uint32_t blk = has_sb(a) ? block_of[island_of[(uint32_t)a]] : has_sb(b) ? block_of[island_of[(uint32_t)b]] : 0u;  // (no SolverBody on either side: touches no body, any block)
            return (size_t)blk * AVN_GRAPH_COLOR_COUNT + (c == AVN_COLOR_OVERFLOW_INDEX ? 0u : c + 1u);
        };
        for (uint32_t c = 0; c < AVN_GRAPH_COLOR_COUNT; ++c)
            for (uint32_t m = color_offsets[c]; m < color_offsets[c + 1]; ++m) ++col_off[key_of(m, c) + 1];
        for (size_t i = 1; i < col_off.size(); ++i) col_off[i] += col_off[i - 1];
        std::vector<uint32_t> next(col_off.begin(), col_off.end() - 1);
        ent.resize((size_t)M * 2);
        for (uint32_t c = 0; c < AVN_GRAPH_COLOR_COUNT; ++c)
            for (uint32_t m = color_offsets[c]; m < color_offsets[c + 1]; ++m) {
                int32_t a = h_m_body1[m], b = h_m_body2[m];
                uint32_t e = next[key_of(m, c)]++;
                ent[2 * (size_t)e] = m;
                ent[2 * (size_t)e + 1] = (has_sb(a) ? slot[(uint32_t)a] : 0u) | (has_sb(b) ? slot[(uint32_t)b] : 0u) << 16;
            }
        // one pinned staging block -> one async copy on the solver's stream (the consumer); no synchronisation: the stream
        // was idle when the previous block went up (rebuild_incidence / the narrow-phase read-back synchronise it every step)
        const size_t w0 = body_off.size(), w1 = bodies.size(), w2 = col_off.size(), w3 = ent.size();
        const size_t o1 = (w0 + 63) & ~(size_t)63, o2 = o1 + ((w1 + 63) & ~(size_t)63), o3 = o2 + ((w2 + 63) & ~(size_t)63), words = o3 + w3;
        ALLOC(pin_islands.ensure(words * 4));
        uint32_t* h = (uint32_t*)pin_islands.p;
        std::memcpy(h, body_off.data(), w0 * 4); std::memcpy(h + o1, bodies.data(), w1 * 4);
        std::memcpy(h + o2, col_off.data(), w2 * 4); std::memcpy(h + o3, ent.data(), w3 * 4);
        if (words * 4 > b_isl_bodies.cap) HIPCHK(hipStreamSynchronize(stream));   // growing frees the old block: nothing may still read it
        ALLOC(b_isl_bodies.ensure(words * 4));
        HIPCHK(hipMemcpyAsync(b_isl_bodies.p, h, words * 4, hipMemcpyHostToDevice, stream));
        uint32_t* d = b_isl_bodies.as<uint32_t>();
        islands = IslandBlocks{d, d + o1, d + o2, (const uint2*)(d + o3), n_blocks, max_bodies, lm_pad, cache_records ? 1u : 0u};
        island_mode = true;
        return AVN_OK;
    }
    avn_status impulses_download(const avn_impulses_out* o) override {
        if (!o) return AVN_ERR_BAD_ARG;
        { const avn_status sm = materialize_impulses(); if (sm != AVN_OK) return sm; }
        size_t M = dw.n_manifolds;
        T *a, *b, *c;
        StagePlan plan(*this);
        plan.out(o->warm_start_normal_impulse, 4 * M, &a); plan.out(o->warm_start_tangent_impulse, 8 * M, &b);
        plan.out(o->normal_impulse, 4 * M, &c);
        COMMIT(plan);
        if (use_handles && !pipe_dev) {
            // handle lists (host bookkeeping): store_contact_impulses scattered the impulses into the contact table, and DW::mp_w holds only what k_store_contact_impulses
            // wrote -- the points of manifolds that generated a constraint; every other slot was never written by anyone.  Answer from the rows the handles name: points
            // beyond a row's count read as zero, as avn_contacts_download gives them.  (The device closed loop keeps the arrays: its n_manifolds is an upper bound of the list.)
            ContactsStage<T> rows;
            std::memset(&rows, 0, sizeof rows);
            rows.warm_n = a; rows.warm_t = b; rows.normal_impulse = c;
            if (M) launch_unpack_contacts<T>(ct, b_handles.as<uint32_t>(), (uint32_t)M, rows, stream);
        } else
        launch_unpack_impulses<T>(dw, a, b, c, lvl_perm(), stream);
        HIPCHK(hipGetLastError());
        FINISH(plan);
        HIPCHK(hipStreamSynchronize(stream));
        return AVN_OK;
    }
    avn_status constraints_download(const avn_constraints_out* o) override {
        if (!o) return AVN_ERR_BAD_ARG;
        size_t M = dw.n_manifolds;
        ConstraintsStage<T> s;
        StagePlan plan(*this);
        SOUT(point_count, o->point_count, M); SOUT(softness_non_dynamic, o->softness_non_dynamic, M);
        SOUT(relative_dominance, o->relative_dominance, M); SOUT(tangent1, o->tangent1, 3 * M);
        SOUT(anchor1, o->anchor1, 12 * M); SOUT(initial_separation, o->initial_separation, 4 * M);
        SOUT(normal_impulse, o->normal_impulse, 4 * M); SOUT(total_impulse, o->total_impulse, 4 * M);
        SOUT(normal_effective_mass, o->normal_effective_mass, 4 * M); SOUT(tangent_impulse, o->tangent_impulse, 8 * M);
        SOUT(tangent_k, o->tangent_effective_inverse_mass, 12 * M);
        COMMIT(plan);
        if (plan.bytes()) HIPCHK(hipMemsetAsync(stage.p, 0, plan.bytes(), stream));  // absent constraints read back as zeros
        launch_unpack_constraints<T>(dw, s, lvl_perm(), stream);
        HIPCHK(hipGetLastError());
        FINISH(plan);
        HIPCHK(hipStreamSynchronize(stream));
        return AVN_OK;
    }

