// world/spatial.hpp -- fragment of the body of `template <class T> struct World` (avn_world.hip includes it inside the class):
// SpatialQueryPlugin (spatial_query/mod.rs:190-212) on the device -- include/avian_mi355x_spatial.h.  avn_spatial_update builds the LBVH of
// k_spatial.hip from the poses in HBM; the queries stage their inputs, run one traversal launch and copy the answers back.  The casters
// (RayCaster / ShapeCaster) keep their definitions and answers on the device: avn_spatial_casters_run only enqueues.

    SP<T> sp{};
    DevBuf b_sp_pos, b_sp_rot, b_sp_he, b_sp_info, b_sp_smin, b_sp_smax, b_sp_bmin, b_sp_bmax, b_sp_child, b_sp_parent, b_sp_leaf, b_sp_arr, b_sp_bounds,
        b_sp_keys_a, b_sp_vals_a, b_sp_keys_b, b_sp_vals_b, b_sp_hist, b_sp_block_sums, b_sp_stats,
        b_sp_crec, b_sp_ccount,   // depenetrate's contact records [n * AVN_SPATIAL_MAX_HITS] and counts [n]
        b_sl_pos, b_sl_vel, b_sl_time, b_sl_move, b_sl_pred, b_sl_flags, b_sl_iters, b_sl_hits, b_sl_nplanes, b_sl_planes, b_sl_cfg, b_sl_mh,   // move_and_slide's per-character state
        b_mv_pend, b_mv_pcount;   // cast_move's hand-over: the colliders overlapping each query at its start [n * AVN_SPATIAL_MAX_HITS], their counts [n]
    uint32_t sp_cap = 0;
    bool sp_valid = false;      // a snapshot exists and no table changed since (bodies / colliders / collider transforms uploads and avn_despawn clear it)
    uint32_t sp_host = 0;       // the colliders the snapshot leaves out: AVN_SHAPE_HOST; AVN_SHAPE_CAPSULE unless sp_capsules is set; AVN_SHAPE_TRIANGLE unless sp_triangles is
    bool sp_capsules = false;   // avn_spatial_capsule_colliders_set: capsule colliders are candidates of the queries (sticky, off by default)
    bool sp_ccap = false;       // the snapshot holds capsule colliders as candidates: every traversal launch takes its CCAP instantiation
    bool sp_triangles = false;  // avn_spatial_triangle_colliders_set: triangle colliders are candidates of the queries (sticky, off by default)
    bool sp_ctri = false;       // the snapshot holds triangle colliders as candidates: every traversal launch takes its CTRI instantiation
    // the triangle table the CTRI launches read (the world's, not a copy: avn_colliders_upload and avn_collider_triangles_upload clear sp_valid, and sp_check
    // lets no query through until the next update has taken the new pointer)
    const V* sp_tri_table() const { return sp_ctri ? bp.col_tri : nullptr; }
    unsigned long long sp_visits[3] = {0, 0, 0};   // last query call: node boxes tested, exact tests, stack overflow

    avn_status sp_grow(uint32_t C) {
        if (sp_cap && C <= sp_cap) return AVN_OK;
        HIPCHK(hipStreamSynchronize(stream));   // (the old buffers may still be read by an update in flight)
        const size_t cc = std::max<size_t>({(size_t)C, (size_t)sp_cap + sp_cap / 2, 64});
        GROW(b_sp_pos, cc, sp.pos); GROW(b_sp_rot, cc, sp.rot); GROW(b_sp_he, cc, sp.he); GROW(b_sp_info, cc, sp.info);
        GROW(b_sp_smin, cc, sp.smin); GROW(b_sp_smax, cc, sp.smax);
        GROW(b_sp_bmin, 2 * cc, sp.bmin); GROW(b_sp_bmax, 2 * cc, sp.bmax); GROW(b_sp_child, cc, sp.child); GROW(b_sp_parent, 2 * cc, sp.parent);
        GROW(b_sp_leaf, cc, sp.leaf_col); GROW(b_sp_arr, cc, sp.arrivals); GROW(b_sp_bounds, 8, sp.bounds);
        GROW(b_sp_keys_a, cc, sp.keys_a); GROW(b_sp_vals_a, cc, sp.vals_a); GROW(b_sp_keys_b, cc, sp.keys_b); GROW(b_sp_vals_b, cc, sp.vals_b);
        GROW(b_sp_hist, (size_t)256 * radix_blocks((uint32_t)cc) + 256, sp.hist);
        GROW(b_sp_block_sums, scan_block_sums_needed(256 * radix_blocks((uint32_t)cc)) + 16, sp.block_sums);
        HIPCHK(hipMemset(b_sp_block_sums.p, 0, b_sp_block_sums.cap));   // the one-launch scan's state: zero once, self-cleaning afterwards (avn_scan.h)
        ALLOC(b_sp_stats.ensure(4 * sizeof(unsigned long long)));
        sp_cap = (uint32_t)cc;
        return AVN_OK;
    }

    avn_status spatial_update() override {
        if (!have_bodies || !have_colliders) { error = "spatial_update: before bodies_upload / colliders_upload"; return AVN_ERR_STATE; }
        if (despawn_needs_bodies || despawn_needs_colliders) { error = "spatial_update: avn_despawn is still waiting for avn_bodies_upload / avn_colliders_upload"; return AVN_ERR_STATE; }
        if (!sp_valid) cs_ran = false;   // (the tables changed since the last casters run: its results name the old ones)
        const uint32_t C = bp.n_colliders;
        avn_status st = sp_grow(C);
        if (st != AVN_OK) return st;
        if (sp_triangles && (st = tri_need_table()) != AVN_OK) return st;   // (the CTRI snapshot reads BP::col_tri)
        sp.n = C;
        sp_ccap = sp_capsules && cap_count != 0;   // (a world without a capsule, or with the switch off, launches what it always has)
        sp_ctri = sp_triangles && tri_count != 0 && bp.col_tri != nullptr;   // (likewise for triangles)
        launch_spatial_build<T>(dw, bp, sp, stream, sp_ccap, tri_count != 0, sp_ctri);
        HIPCHK(hipGetLastError());
        sp_host = (uint32_t)hs_slots.size() + (sp_capsules ? 0u : cap_count) + (sp_triangles ? 0u : tri_count);   // (with their switch off triangle colliders are left out exactly as host shapes are)
        sp_valid = true;
        return AVN_OK;
    }

    avn_status spatial_triangle_colliders_set(uint32_t enabled) override {
        sp_triangles = enabled != 0;
        sp_valid = false;   // (the snapshot was built under the old rule: avn_spatial_update again)
        return AVN_OK;
    }

    avn_status spatial_capsule_colliders_set(uint32_t enabled) override {
        sp_capsules = enabled != 0;
        sp_valid = false;   // (the snapshot was built under the old rule: avn_spatial_update again)
        return AVN_OK;
    }

    avn_status sp_check(uint32_t flags) {
        if (!sp_valid) { error = "spatial query: no avn_spatial_update since the tables last changed"; return AVN_ERR_STATE; }
        if (sp_host && tri_count && !sp_triangles && !(flags & AVN_SPATIAL_SKIP_HOST_SHAPES)) {
            error = "spatial query: the snapshot holds AVN_SHAPE_TRIANGLE colliders (and possibly AVN_SHAPE_HOST / AVN_SHAPE_CAPSULE ones), which the queries have no device geometry for (AVN_SPATIAL_SKIP_HOST_SHAPES leaves them out)";
            return AVN_ERR_STATE;
        }
        if (sp_host && !(flags & AVN_SPATIAL_SKIP_HOST_SHAPES)) {
            error = sp_capsules ? "spatial query: the snapshot holds AVN_SHAPE_HOST colliders, which the queries have no device geometry for (AVN_SPATIAL_SKIP_HOST_SHAPES leaves them out)"
                                : "spatial query: the snapshot holds AVN_SHAPE_HOST or AVN_SHAPE_CAPSULE colliders, which the queries have no device geometry for (AVN_SPATIAL_SKIP_HOST_SHAPES leaves them out; avn_spatial_capsule_colliders_set makes capsules candidates)";
            return AVN_ERR_STATE;
        }
        return AVN_OK;
    }
    // the shared excluded list, sorted on the host (read back first when it is a device array)
    avn_status sp_excluded(const avn_spatial_filter& f, bool dev, std::vector<uint32_t>& ex) {
        if (f.n_excluded && !f.excluded) { error = "spatial query: filter.excluded is NULL"; return AVN_ERR_BAD_ARG; }
        ex.resize(f.n_excluded);
        if (f.n_excluded) {
            if (dev) HIPCHK(hipMemcpy(ex.data(), f.excluded, (size_t)f.n_excluded * 4, hipMemcpyDeviceToHost));
            else std::memcpy(ex.data(), f.excluded, (size_t)f.n_excluded * 4);
            std::sort(ex.begin(), ex.end());
        }
        return AVN_OK;
    }
    // the filter of a call: the per-query masks are the caller's (host or device), the sorted excluded list is always staged
    void sp_filter_in(StagePlan& plan, SQ<T>& q, const avn_spatial_filter& f, uint32_t n, const std::vector<uint32_t>& ex) {
        plan.in(f.mask, n, &q.mask);
        plan.staged(ex.data(), ex.size(), &q.excluded);
        q.n_excluded = (uint32_t)ex.size();
    }
    // Whether a call may hold AVN_SHAPE_CAPSULE query shapes, which the kernels' second (CAPSULE) instantiations answer: the host's kinds are
    // scanned, a device array is not read back (the second launch always goes; its lanes leave at once unless their query is a capsule).
    static bool sp_any_capsule(const uint8_t* shape, uint32_t n, bool dev) {
        if (dev) return n != 0;
        for (uint32_t i = 0; i < n; ++i) if (shape[i] == AVN_SHAPE_CAPSULE) return true;
        return false;
    }
    avn_status sp_run(SQ<T>& q, int kind, bool capsule = false) {
        q.stats = b_sp_stats.as<unsigned long long>();
        launch_spatial_query<T>(sp, q, kind, stream, capsule, sp_ccap, sp_tri_table());
        HIPCHK(hipGetLastError());
        return AVN_OK;
    }
    avn_status sp_finish() {
        HIPCHK(hipMemcpyAsync(sp_visits, b_sp_stats.p, sizeof sp_visits, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        if (sp_visits[2] & 2ull) { error = "spatial query: a move overlaps more than AVN_SPATIAL_MAX_HITS colliders at its start"; return AVN_ERR_CAPACITY; }
        if (sp_visits[2]) { error = "spatial query: traversal stack overflow"; return AVN_ERR_CAPACITY; }
        return AVN_OK;
    }

    avn_status spatial_cast_rays(const avn_spatial_rays* r, uint32_t max_hits, const avn_spatial_hits_out* out) override {
        if (!r || !out) { error = "spatial ray query: null argument"; return AVN_ERR_BAD_ARG; }
        const uint32_t n = r->count;
        const bool many = max_hits != 0;
        if (n && (!r->origin || !r->direction || !r->max_distance || !r->solid || !out->hits || (many && !out->count))) { error = "spatial ray query: null array"; return AVN_ERR_BAD_ARG; }
        if (max_hits > AVN_SPATIAL_MAX_HITS) { error = "spatial_ray_hits: max_hits above AVN_SPATIAL_MAX_HITS"; return AVN_ERR_BAD_ARG; }
        avn_status st = sp_check(r->flags);
        if (st != AVN_OK) return st;
        const bool dev = (r->flags & AVN_SPATIAL_DEVICE_POINTERS) != 0;
        std::vector<uint32_t> ex;
        if ((st = sp_excluded(r->filter, dev, ex)) != AVN_OK) return st;
        const size_t n_rec = (size_t)n * (many ? max_hits : 1);
        SQ<T> q{};
        q.n = n; q.cap = max_hits;
        StagePlan plan(*this, dev);
        plan.in(r->origin, 3 * (size_t)n, &q.a); plan.in(r->direction, 3 * (size_t)n, &q.b);
        plan.in(r->max_distance, n, &q.max_distance); plan.in(r->solid, n, &q.solid);
        sp_filter_in(plan, q, r->filter, n, ex);
        plan.out(out->hits, n_rec, &q.hits);
        if (many) plan.out(out->count, n, &q.count);
        COMMIT(plan);
        if ((st = sp_run(q, many ? SPQ_HITS : SPQ_CLOSEST)) != AVN_OK) return st;
        FINISH(plan);
        return sp_finish();
    }

    // point (kind SPQ_POINTS: a = points) and box (SPQ_AABBS: a = mins, b = maxs) intersections
    avn_status sp_ids(int kind, uint32_t n, uint32_t flags, const void* a, const void* b, const avn_spatial_filter& f, uint32_t cap, const avn_spatial_ids_out* out) {
        if (!out) { error = "spatial query: null argument"; return AVN_ERR_BAD_ARG; }
        if (n && (!a || (kind == SPQ_AABBS && !b) || !out->count || (cap && !out->collider))) { error = "spatial query: null array"; return AVN_ERR_BAD_ARG; }
        avn_status st = sp_check(flags);
        if (st != AVN_OK) return st;
        const bool dev = (flags & AVN_SPATIAL_DEVICE_POINTERS) != 0;
        std::vector<uint32_t> ex;
        if ((st = sp_excluded(f, dev, ex)) != AVN_OK) return st;
        const size_t n_ids = (size_t)n * cap;
        SQ<T> q{};
        q.n = n; q.cap = cap;
        StagePlan plan(*this, dev);
        plan.in(a, 3 * (size_t)n, &q.a);
        if (kind == SPQ_AABBS) plan.in(b, 3 * (size_t)n, &q.b);
        sp_filter_in(plan, q, f, n, ex);
        plan.out(out->collider, n_ids, &q.ids); plan.out(out->count, n, &q.count);
        COMMIT(plan);
        if ((st = sp_run(q, kind)) != AVN_OK) return st;
        FINISH(plan);
        return sp_finish();
    }
    avn_status spatial_point_intersections(const avn_spatial_points* p, uint32_t cap, const avn_spatial_ids_out* out) override {
        if (!p) { error = "spatial_point_intersections: null argument"; return AVN_ERR_BAD_ARG; }
        return sp_ids(SPQ_POINTS, p->count, p->flags, p->point, nullptr, p->filter, cap, out);
    }
    avn_status spatial_aabb_intersections(const avn_spatial_aabbs* b, uint32_t cap, const avn_spatial_ids_out* out) override {
        if (!b) { error = "spatial_aabb_intersections: null argument"; return AVN_ERR_BAD_ARG; }
        return sp_ids(SPQ_AABBS, b->count, b->flags, b->min, b->max, b->filter, cap, out);
    }
    avn_status spatial_project_points(const avn_spatial_solid_points* p, const avn_spatial_projections_out* out) override {
        if (!p || !out) { error = "spatial_project_points: null argument"; return AVN_ERR_BAD_ARG; }
        const uint32_t n = p->count;
        if (n && (!p->point || !p->solid || !out->projection)) { error = "spatial_project_points: null array"; return AVN_ERR_BAD_ARG; }
        avn_status st = sp_check(p->flags);
        if (st != AVN_OK) return st;
        const bool dev = (p->flags & AVN_SPATIAL_DEVICE_POINTERS) != 0;
        std::vector<uint32_t> ex;
        if ((st = sp_excluded(p->filter, dev, ex)) != AVN_OK) return st;
        SQ<T> q{};
        q.n = n;
        StagePlan plan(*this, dev);
        plan.in(p->point, 3 * (size_t)n, &q.a); plan.in(p->solid, n, &q.solid);
        sp_filter_in(plan, q, p->filter, n, ex);
        plan.out(out->projection, n, &q.proj);
        COMMIT(plan);
        if ((st = sp_run(q, SPQ_PROJECT)) != AVN_OK) return st;
        FINISH(plan);
        return sp_finish();
    }
    avn_status spatial_shape_intersections(const avn_spatial_shapes* s, uint32_t cap, const avn_spatial_ids_out* out) override {
        if (!s || !out) { error = "spatial_shape_intersections: null argument"; return AVN_ERR_BAD_ARG; }
        const uint32_t n = s->count;
        if (n && (!s->shape || !s->half_extents || !s->position || !s->rotation || !out->count || (cap && !out->collider))) { error = "spatial_shape_intersections: null array"; return AVN_ERR_BAD_ARG; }
        avn_status st = sp_check(s->flags);
        if (st != AVN_OK) return st;
        const bool dev = (s->flags & AVN_SPATIAL_DEVICE_POINTERS) != 0;
        std::vector<uint32_t> ex;
        if ((st = sp_excluded(s->filter, dev, ex)) != AVN_OK) return st;
        const size_t n_ids = (size_t)n * cap;
        SQ<T> q{};
        q.cap = cap;
        StagePlan plan(*this, dev);
        sp_shape_inputs(plan, q, n, s->shape, s->half_extents, s->position, s->rotation, s->filter, ex);
        plan.out(out->collider, n_ids, &q.ids); plan.out(out->count, n, &q.count);
        COMMIT(plan);
        if ((st = sp_run(q, SPQ_SHAPES, sp_any_capsule(s->shape, n, dev))) != AVN_OK) return st;
        FINISH(plan);
        return sp_finish();
    }
    // cast_shapes (max_hits == 0: the closest hit per cast) and shape_hits (the max_hits nearest, plus the true count)
    avn_status spatial_cast_shapes(const avn_spatial_shape_casts* s, uint32_t max_hits, const avn_spatial_shape_hits_out* out) override {
        if (!s || !out) { error = "spatial shape cast: null argument"; return AVN_ERR_BAD_ARG; }
        const uint32_t n = s->count;
        const bool many = max_hits != 0;
        if (n && (!s->shape || !s->half_extents || !s->position || !s->rotation || !s->direction || !s->max_distance || !out->hits || (many && !out->count))) {
            error = "spatial shape cast: null array"; return AVN_ERR_BAD_ARG;
        }
        if (max_hits > AVN_SPATIAL_MAX_HITS) { error = "spatial_shape_hits: max_hits above AVN_SPATIAL_MAX_HITS"; return AVN_ERR_BAD_ARG; }
        avn_status st = sp_check(s->flags);
        if (st != AVN_OK) return st;
        const bool dev = (s->flags & AVN_SPATIAL_DEVICE_POINTERS) != 0;
        std::vector<uint32_t> ex;
        if ((st = sp_excluded(s->filter, dev, ex)) != AVN_OK) return st;
        const size_t n_rec = (size_t)n * (many ? max_hits : 1);
        SQ<T> q{};
        q.n = n; q.cap = max_hits;
        StagePlan plan(*this, dev);
        plan.in(s->shape, n, &q.shape); plan.in(s->half_extents, 3 * (size_t)n, &q.he);
        plan.in(s->position, 3 * (size_t)n, &q.a); plan.in(s->rotation, 4 * (size_t)n, &q.rot);
        plan.in(s->direction, 3 * (size_t)n, &q.b); plan.in(s->max_distance, n, &q.max_distance);
        sp_filter_in(plan, q, s->filter, n, ex);
        plan.out(out->hits, n_rec, &q.cast);
        if (many) plan.out(out->count, n, &q.count);
        COMMIT(plan);
        if ((st = sp_run(q, many ? SPQ_CAST_HITS : SPQ_CAST, sp_any_capsule(s->shape, n, dev))) != AVN_OK) return st;
        FINISH(plan);
        return sp_finish();
    }
    // the query-shape fields (the SPQ_SHAPES fields of q) shared by shape_intersections, shape_contacts, depenetrate, cast_moves and move_and_slide
    void sp_shape_inputs(StagePlan& plan, SQ<T>& q, uint32_t n, const uint8_t* shape, const void* he, const void* pos, const void* rot, const avn_spatial_filter& f,
                         const std::vector<uint32_t>& ex) {
        q.n = n;
        plan.in(shape, n, &q.shape); plan.in(he, 3 * (size_t)n, &q.he); plan.in(pos, 3 * (size_t)n, &q.a); plan.in(rot, 4 * (size_t)n, &q.rot);
        sp_filter_in(plan, q, f, n, ex);
        q.stats = b_sp_stats.as<unsigned long long>();
    }
    // MoveAndSlide::intersections: the deepest contact per collider within the prediction distance, ascending collider index
    avn_status spatial_shape_contacts(const avn_spatial_shape_contact_queries* s, uint32_t cap, const avn_spatial_shape_contacts_out* out) override {
        if (!s || !out) { error = "spatial_shape_contacts: null argument"; return AVN_ERR_BAD_ARG; }
        const uint32_t n = s->count;
        if (n && (!s->shape || !s->half_extents || !s->position || !s->rotation || !s->prediction_distance || !out->count || (cap && !out->contacts))) {
            error = "spatial_shape_contacts: null array"; return AVN_ERR_BAD_ARG;
        }
        if (cap > AVN_SPATIAL_MAX_HITS) { error = "spatial_shape_contacts: cap above AVN_SPATIAL_MAX_HITS"; return AVN_ERR_BAD_ARG; }
        avn_status st = sp_check(s->flags);
        if (st != AVN_OK) return st;
        const bool dev = (s->flags & AVN_SPATIAL_DEVICE_POINTERS) != 0;
        std::vector<uint32_t> ex;
        if ((st = sp_excluded(s->filter, dev, ex)) != AVN_OK) return st;
        const size_t n_rec = (size_t)n * cap;
        SC<T> sc{};
        StagePlan plan(*this, dev);
        sp_shape_inputs(plan, sc.q, n, s->shape, s->half_extents, s->position, s->rotation, s->filter, ex);
        plan.in(s->prediction_distance, n, &sc.prediction);
        sc.q.cap = cap;
        sc.skip_sensors = (s->flags & AVN_SPATIAL_SKIP_SENSORS) ? 1u : 0u;
        sc.pad_unused = 1u;
        plan.out(out->contacts, n_rec, &sc.rec); plan.out(out->count, n, &sc.q.count);
        COMMIT(plan);
        launch_spatial_contacts<T>(sp, sc, stream, true, sp_any_capsule(s->shape, n, dev), sp_ccap, sp_tri_table());
        HIPCHK(hipGetLastError());
        FINISH(plan);
        return sp_finish();
    }
    // MoveAndSlide::depenetrate: the contacts with prediction skin_width into a buffer the world keeps, then k_sp_depenetrate over them
    avn_status spatial_depenetrate(const avn_spatial_shapes* s, const avn_spatial_depenetration_config* cfg, const avn_spatial_depenetrations_out* out) override {
        if (!s || !cfg || !out) { error = "spatial_depenetrate: null argument"; return AVN_ERR_BAD_ARG; }
        const uint32_t n = s->count;
        if (n && (!s->shape || !s->half_extents || !s->position || !s->rotation || !out->depenetration)) { error = "spatial_depenetrate: null array"; return AVN_ERR_BAD_ARG; }
        avn_status st = sp_check(s->flags);
        if (st != AVN_OK) return st;
        const bool dev = (s->flags & AVN_SPATIAL_DEVICE_POINTERS) != 0;
        std::vector<uint32_t> ex;
        if ((st = sp_excluded(s->filter, dev, ex)) != AVN_OK) return st;
        SpatialDepenetration<T>* d_out;
        StagePlan plan(*this, dev);
        plan.out(out->depenetration, n, &d_out);
        if (cfg->iterations == 0) {
            COMMIT(plan);
            // depenetration disabled: zero vectors, no traversal (every byte of a record is 0)
            if (n) HIPCHK(hipMemsetAsync(d_out, 0, (size_t)n * sizeof(SpatialDepenetration<T>), stream));
            HIPCHK(hipMemsetAsync(b_sp_stats.p, 0, 4 * sizeof(unsigned long long), stream));
        } else {
            SC<T> sc{};
            uint32_t* d_count;
            GROW(b_sp_crec, std::max<size_t>((size_t)n * AVN_SPATIAL_MAX_HITS, 1), sc.rec);
            GROW(b_sp_ccount, std::max<size_t>(n, 1), d_count);
            sp_shape_inputs(plan, sc.q, n, s->shape, s->half_extents, s->position, s->rotation, s->filter, ex);
            COMMIT(plan);
            sc.q.cap = AVN_SPATIAL_MAX_HITS;
            sc.q.count = d_count;
            sc.prediction = nullptr;
            sc.prediction_all = (T)cfg->skin_width;
            sc.pad_unused = 0u;   // (k_sp_depenetrate reads the first min(count, cap) records only)
            sc.skip_sensors = (s->flags & AVN_SPATIAL_SKIP_SENSORS) ? 1u : 0u;
            launch_spatial_contacts<T>(sp, sc, stream, true, sp_any_capsule(s->shape, n, dev), sp_ccap, sp_tri_table());
            HIPCHK(hipGetLastError());
            SD<T> d{};
            d.n = n; d.rec = sc.rec; d.count = d_count;
            d.skin_width = (T)cfg->skin_width; d.max_error = (T)cfg->max_depenetration_error; d.rejection = (T)cfg->penetration_rejection_threshold;
            d.iterations = cfg->iterations;
            d.out = d_out;
            launch_spatial_depenetrate<T>(d, stream);
            HIPCHK(hipGetLastError());
        }
        FINISH(plan);
        return sp_finish();
    }
    // project_velocity per query: no snapshot, no traversal
    avn_status spatial_project_velocities(const avn_spatial_velocity_projections* p, const avn_spatial_velocities_out* out) override {
        if (!p || !out) { error = "spatial_project_velocities: null argument"; return AVN_ERR_BAD_ARG; }
        const uint32_t n = p->count;
        if (p->stride > AVN_SPATIAL_MAX_PLANES) { error = "spatial_project_velocities: stride above AVN_SPATIAL_MAX_PLANES"; return AVN_ERR_BAD_ARG; }
        if (n && (!p->velocity || !p->normal_count || !out->velocity || (p->stride && !p->normals))) { error = "spatial_project_velocities: null array"; return AVN_ERR_BAD_ARG; }
        const bool dev = (p->flags & AVN_SPATIAL_DEVICE_POINTERS) != 0;
        const size_t n_nrm = (size_t)n * p->stride * 3;
        SV<T> v{};
        v.n = n; v.stride = p->stride;
        StagePlan plan(*this, dev);
        plan.in(p->velocity, 3 * (size_t)n, &v.velocity); plan.in(p->normals, n_nrm, &v.normals); plan.in(p->normal_count, n, &v.count);
        plan.out(out->velocity, 3 * (size_t)n, &v.out);
        COMMIT(plan);
        launch_spatial_project_velocity<T>(v, stream);
        HIPCHK(hipGetLastError());
        FINISH(plan);
        HIPCHK(hipStreamSynchronize(stream));
        return AVN_OK;
    }
    // MoveAndSlide::cast_move per move
    avn_status spatial_cast_moves(const avn_spatial_moves* s, const avn_spatial_move_hits_out* out) override {
        if (!s || !out) { error = "spatial_cast_moves: null argument"; return AVN_ERR_BAD_ARG; }
        const uint32_t n = s->count;
        if (n && (!s->shape || !s->half_extents || !s->position || !s->rotation || !s->movement || !s->skin_width || !out->hits)) { error = "spatial_cast_moves: null array"; return AVN_ERR_BAD_ARG; }
        avn_status st = sp_check(s->flags);
        if (st != AVN_OK) return st;
        const bool dev = (s->flags & AVN_SPATIAL_DEVICE_POINTERS) != 0;
        std::vector<uint32_t> ex;
        if ((st = sp_excluded(s->filter, dev, ex)) != AVN_OK) return st;
        SM<T> m{};
        StagePlan plan(*this, dev);
        sp_shape_inputs(plan, m.q, n, s->shape, s->half_extents, s->position, s->rotation, s->filter, ex);
        plan.in(s->movement, 3 * (size_t)n, &m.movement); plan.in(s->skin_width, n, &m.skin); plan.in(s->self_entity, n, &m.self_entity);
        plan.out(out->hits, n, &m.out);
        COMMIT(plan);
        GROW(b_mv_pend, std::max<size_t>((size_t)n * AVN_SPATIAL_MAX_HITS, 1), m.pending);
        GROW(b_mv_pcount, std::max<size_t>(n, 1), m.pending_count);
        launch_spatial_cast_move<T>(sp, m, true, stream, sp_any_capsule(s->shape, n, dev), sp_ccap, sp_tri_table());
        HIPCHK(hipGetLastError());
        FINISH(plan);
        return sp_finish();
    }
    // MoveAndSlide::move_and_slide per character: a fixed sequence of launches over the state buffers, no read-back inside the loop
    avn_status spatial_move_and_slide(const avn_spatial_characters* s, const avn_spatial_move_and_slide_config* cfg, uint32_t hit_cap, const avn_spatial_slides_out* out) override {
        if (!s || !cfg || !out) { error = "spatial_move_and_slide: null argument"; return AVN_ERR_BAD_ARG; }
        const uint32_t n = s->count;
        if (cfg->n_planes > AVN_SPATIAL_MAX_PLANES || cfg->max_planes > AVN_SPATIAL_MAX_PLANES || cfg->move_and_slide_iterations > AVN_SPATIAL_MAX_SLIDE_ITERATIONS ||
            hit_cap > AVN_SPATIAL_MAX_HITS || (cfg->n_planes && !cfg->planes)) {
            error = "spatial_move_and_slide: n_planes / max_planes above AVN_SPATIAL_MAX_PLANES, iterations above AVN_SPATIAL_MAX_SLIDE_ITERATIONS, hit_cap above AVN_SPATIAL_MAX_HITS or planes NULL";
            return AVN_ERR_BAD_ARG;
        }
        if (n && (!s->shape || !s->half_extents || !s->position || !s->rotation || !s->velocity || !out->slides || (hit_cap && !out->hits))) { error = "spatial_move_and_slide: null array"; return AVN_ERR_BAD_ARG; }
        avn_status st = sp_check(s->flags);
        if (st != AVN_OK) return st;
        const bool dev = (s->flags & AVN_SPATIAL_DEVICE_POINTERS) != 0;
        std::vector<uint32_t> ex;
        if ((st = sp_excluded(s->filter, dev, ex)) != AVN_OK) return st;
        const size_t n_hits = (size_t)n * hit_cap;
        SC<T> sc{};
        SL<T> l{};
        const uint32_t* self = nullptr;
        StagePlan plan(*this, dev);
        sp_shape_inputs(plan, sc.q, n, s->shape, s->half_extents, s->position, s->rotation, s->filter, ex);
        plan.in(s->velocity, 3 * (size_t)n, &l.vel_in); plan.in(s->self_entity, n, &self);
        plan.out(out->slides, n, &l.out); plan.out(out->hits, n_hits, &l.hits);
        COMMIT(plan);
        l.n = n; l.hit_cap = hit_cap; l.n_planes = cfg->n_planes; l.max_planes = cfg->max_planes; l.depen_iterations = cfg->depenetration_iterations;
        l.shape = sc.q.shape; l.he = sc.q.he; l.pos_in = sc.q.a; l.rot = sc.q.rot;
        const size_t nn = std::max<size_t>(n, 1);
        uint32_t* d_count;
        SpatialMoveHit<T>* d_mh;
        float* d_cfg_planes;
        GROW(b_sp_crec, nn * AVN_SPATIAL_MAX_HITS, sc.rec);
        GROW(b_sp_ccount, nn, d_count);
        GROW(b_sl_pos, 3 * nn, l.pos); GROW(b_sl_vel, 3 * nn, l.vel); GROW(b_sl_time, nn, l.time_left); GROW(b_sl_move, 3 * nn, l.movement); GROW(b_sl_pred, nn, l.pred);
        GROW(b_sl_flags, nn, l.flags); GROW(b_sl_iters, nn, l.iters); GROW(b_sl_hits, nn, l.hit_count); GROW(b_sl_nplanes, nn, l.plane_count);
        GROW(b_sl_planes, nn * SP_SLIDE_PLANES * 3, l.planes); GROW(b_sl_cfg, 3 * AVN_SPATIAL_MAX_PLANES, d_cfg_planes); GROW(b_sl_mh, nn, d_mh);
        if (cfg->n_planes) HIPCHK(hipMemcpyAsync(d_cfg_planes, cfg->planes, (size_t)cfg->n_planes * 3 * sizeof(float), hipMemcpyHostToDevice, stream));
        l.cfg_planes = d_cfg_planes;
        l.delta_time = (T)cfg->delta_time; l.skin = (T)cfg->skin_width; l.threshold = (T)cfg->plane_similarity_dot_threshold;
        l.max_error = (T)cfg->max_depenetration_error; l.rejection = (T)cfg->penetration_rejection_threshold;
        l.rec = sc.rec; l.count = d_count; l.mh = d_mh;
        // the sub-queries read the state: positions from l.pos, never sensors, never the character's own entity
        sc.q.a = l.pos; sc.q.cap = AVN_SPATIAL_MAX_HITS; sc.q.count = d_count;
        sc.skip_sensors = 1u; sc.pad_unused = 0u; sc.self_entity = self;
        SM<T> m{};
        GROW(b_mv_pend, nn * AVN_SPATIAL_MAX_HITS, m.pending);
        GROW(b_mv_pcount, nn, m.pending_count);
        m.q = sc.q; m.movement = l.movement; m.skin = nullptr; m.skin_all = l.skin; m.self_entity = self; m.state = l.flags; m.out = d_mh;
        HIPCHK(hipMemsetAsync(b_sp_stats.p, 0, 4 * sizeof(unsigned long long), stream));
        const bool capsule = sp_any_capsule(s->shape, n, dev);   // (every traversal launch of the loop gets its CAPSULE instantiation behind it)
        auto depenetrate = [&]() {
            if (cfg->depenetration_iterations) { sc.prediction = nullptr; sc.prediction_all = l.skin; launch_spatial_contacts<T>(sp, sc, stream, false, capsule, sp_ccap, sp_tri_table()); }
            launch_spatial_slide_phase<T>(l, SPL_DEPENETRATE, stream);
        };
        launch_spatial_slide_phase<T>(l, SPL_BEGIN, stream);
        depenetrate();
        for (uint32_t it = 0; it < cfg->move_and_slide_iterations; ++it) {
            l.iteration = it;
            launch_spatial_slide_phase<T>(l, SPL_SWEEP, stream);
            launch_spatial_cast_move<T>(sp, m, false, stream, capsule, sp_ccap, sp_tri_table());
            launch_spatial_slide_phase<T>(l, SPL_ADVANCE, stream);
            sc.prediction = l.pred;
            launch_spatial_contacts<T>(sp, sc, stream, false, capsule, sp_ccap, sp_tri_table());
            launch_spatial_slide_phase<T>(l, SPL_PLANES, stream);
        }
        depenetrate();
        launch_spatial_slide_phase<T>(l, SPL_END, stream);
        HIPCHK(hipGetLastError());
        FINISH(plan);
        return sp_finish();
    }
    // ---- casters (include/avian_mi355x_spatial.h "Casters") ----
    // One table per kind: the definitions in one device allocation (`def`), the re-aimed queries and the records in another (`res`).  The casters
    // with k = min(max_hits, hit_cap) <= 1 run in the closest-hit kernel, the others in the nearest-k kernel: two index lists made at upload.
    struct CasterDef {   // the fields of avn_spatial_ray_casters / avn_spatial_shape_casters
        uint32_t count, hit_cap;
        const uint8_t* anchor_kind; const uint32_t* anchor; const void* origin; const float* direction; const void* max_distance; const uint32_t* max_hits;
        const uint8_t *solid, *shape; const void *half_extents, *shape_rotation;
        const uint8_t* enabled; const uint32_t *mask, *self_entity, *excluded_offset, *excluded;
    };
    struct CasterSet {
        uint32_t n = 0, hit_cap = 0, n_closest = 0, n_many = 0;
        bool any_body = false, any_collider = false, any_capsule = false;   // any_capsule: a definition is an AVN_SHAPE_CAPSULE (the casts' second launch)
        uint32_t max_body = 0, max_collider = 0;   // the largest anchors, checked against the tables before every run
        DevBuf def, res;
        SCA<T> a{};
        SQ<T> q{};                                 // every field but n / index / stats
        const uint32_t *index_closest = nullptr, *index_many = nullptr;
        void* records = nullptr;                   // SpatialHit<T> / SpatialShapeHit<T> [n * hit_cap]
    };
    CasterSet cs_ray, cs_shape;
    DevBuf b_cs_stats;          // the run's own traversal counters: queries between a run and its getters do not disturb them
    bool cs_ran = false;        // a run's results are on the device and the snapshot they answer against is still valid

    void casters_clear() { cs_ray.n = cs_shape.n = 0; cs_ran = false; }

    avn_status casters_upload(CasterSet& cs, const CasterDef& d, bool is_shape, const char* who) {
        cs_ran = false;
        if (d.count == 0) { cs.n = 0; return AVN_OK; }
        const uint32_t n = d.count;
        if (d.hit_cap == 0 || d.hit_cap > AVN_SPATIAL_MAX_HITS) { error = std::string(who) + ": hit_cap must be 1 .. AVN_SPATIAL_MAX_HITS"; return AVN_ERR_BAD_ARG; }
        if (!d.anchor_kind || !d.anchor || !d.origin || !d.direction || !d.max_distance || !d.max_hits || (!is_shape && !d.solid) ||
            (is_shape && (!d.shape || !d.half_extents || !d.shape_rotation))) { error = std::string(who) + ": null array"; return AVN_ERR_BAD_ARG; }
        const uint32_t n_bodies = have_bodies ? dw.n_bodies : 0u, n_colliders = have_colliders ? bp.n_colliders : 0u;
        bool any_body = false, any_collider = false;
        uint32_t max_body = 0, max_collider = 0;
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t k = d.anchor_kind[i], a = d.anchor[i];
            if (k > AVN_SPATIAL_ANCHOR_COLLIDER) { error = std::string(who) + ": unknown anchor kind"; return AVN_ERR_BAD_ARG; }
            if ((k == AVN_SPATIAL_ANCHOR_BODY && a >= n_bodies) || (k == AVN_SPATIAL_ANCHOR_COLLIDER && a >= n_colliders)) {
                error = std::string(who) + ": anchor " + std::to_string(a) + " of caster " + std::to_string(i) + " is outside its table"; return AVN_ERR_BAD_ARG;
            }
            if (k == AVN_SPATIAL_ANCHOR_BODY) { any_body = true; max_body = std::max(max_body, a); }
            if (k == AVN_SPATIAL_ANCHOR_COLLIDER) { any_collider = true; max_collider = std::max(max_collider, a); }
        }
        std::vector<uint32_t> off(n + 1, 0u), ex;
        if (d.excluded_offset) {
            if (d.excluded_offset[0] != 0u) { error = std::string(who) + ": excluded_offset[0] must be 0"; return AVN_ERR_BAD_ARG; }
            for (uint32_t i = 0; i < n; ++i) if (d.excluded_offset[i + 1] < d.excluded_offset[i]) { error = std::string(who) + ": excluded_offset must ascend"; return AVN_ERR_BAD_ARG; }
            if (d.excluded_offset[n] && !d.excluded) { error = std::string(who) + ": excluded is NULL"; return AVN_ERR_BAD_ARG; }
            off.assign(d.excluded_offset, d.excluded_offset + n + 1);
            ex.assign(d.excluded, d.excluded + off[n]);
            for (uint32_t i = 0; i < n; ++i) std::sort(ex.begin() + off[i], ex.begin() + off[i + 1]);
        }
        std::vector<uint32_t> kq(n), self(n, AVN_SPATIAL_MISS), closest, many;
        std::vector<uint8_t> live(n);
        for (uint32_t i = 0; i < n; ++i) {
            kq[i] = std::min(d.max_hits[i], d.hit_cap);
            live[i] = (!d.enabled || d.enabled[i]) && kq[i] != 0u;
            if (d.self_entity) self[i] = d.self_entity[i];
            (kq[i] <= 1u ? closest : many).push_back(i);
        }
        // the definitions: one host image, one copy
        std::vector<uint8_t> img;
        auto put = [&](const void* p, size_t bytes) { const size_t at = al(img.size()); img.resize(at + bytes); if (bytes) std::memcpy(img.data() + at, p, bytes); return at; };
        const size_t o_kind = put(d.anchor_kind, n), o_anchor = put(d.anchor, 4 * (size_t)n), o_origin = put(d.origin, 3 * sizeof(T) * n), o_dir = put(d.direction, 12 * (size_t)n),
                     o_md = put(d.max_distance, sizeof(T) * n), o_solid = is_shape ? 0 : put(d.solid, n), o_shape = is_shape ? put(d.shape, n) : 0,
                     o_he = is_shape ? put(d.half_extents, 3 * sizeof(T) * n) : 0, o_rot = is_shape ? put(d.shape_rotation, 4 * sizeof(T) * n) : 0,
                     o_mask = d.mask ? put(d.mask, 4 * (size_t)n) : 0, o_self = put(self.data(), 4 * (size_t)n), o_off = put(off.data(), 4 * (size_t)(n + 1)),
                     o_ex = put(ex.data(), 4 * ex.size()), o_kq = put(kq.data(), 4 * (size_t)n), o_live = put(live.data(), n),
                     o_closest = put(closest.data(), 4 * closest.size()), o_many = put(many.data(), 4 * many.size());
        const size_t rec = is_shape ? sizeof(SpatialShapeHit<T>) : sizeof(SpatialHit<T>);
        const size_t r_origin = 0, r_dir = r_origin + al(3 * sizeof(T) * n), r_dir_t = r_dir + al(12 * (size_t)n), r_rot = r_dir_t + al(3 * sizeof(T) * n),
                     r_rec = r_rot + al(4 * sizeof(T) * n), r_count = r_rec + al(rec * n * d.hit_cap), r_end = r_count + al(4 * (size_t)n);
        HIPCHK(hipStreamSynchronize(stream));   // (a run in flight may still read the old tables)
        cs.n = 0;
        ALLOC(cs.def.ensure(al(img.size()) + 64));
        ALLOC(cs.res.ensure(r_end));
        HIPCHK(hipMemcpy(cs.def.p, img.data(), img.size(), hipMemcpyHostToDevice));
        const char* D = (const char*)cs.def.p;
        char* R = (char*)cs.res.p;
        SCA<T>& a = cs.a;
        a = SCA<T>{};
        a.n = n; a.anchor_kind = (const uint8_t*)(D + o_kind); a.anchor = (const uint32_t*)(D + o_anchor); a.origin = (const T*)(D + o_origin);
        a.direction = (const float*)(D + o_dir); a.shape_rotation = is_shape ? (const T*)(D + o_rot) : nullptr;
        a.g_origin = (T*)(R + r_origin); a.g_direction = (float*)(R + r_dir); a.g_direction_t = (T*)(R + r_dir_t); a.g_rotation = is_shape ? (T*)(R + r_rot) : nullptr;
        SQ<T>& q = cs.q;
        q = SQ<T>{};
        q.cap = d.hit_cap; q.a = a.g_origin; q.b = a.g_direction_t; q.max_distance = (const T*)(D + o_md);
        q.solid = is_shape ? nullptr : (const uint8_t*)(D + o_solid);
        q.mask = d.mask ? (const uint32_t*)(D + o_mask) : nullptr;
        q.excluded = (const uint32_t*)(D + o_ex); q.n_excluded = 0;
        q.count = (uint32_t*)(R + r_count);
        if (is_shape) { q.shape = (const uint8_t*)(D + o_shape); q.he = (const T*)(D + o_he); q.rot = a.g_rotation; q.cast = (SpatialShapeHit<T>*)(R + r_rec); }
        else q.hits = (SpatialHit<T>*)(R + r_rec);
        q.self_entity = (const uint32_t*)(D + o_self); q.ex_offset = (const uint32_t*)(D + o_off); q.kq = (const uint32_t*)(D + o_kq); q.live = (const uint8_t*)(D + o_live);
        cs.records = R + r_rec;
        cs.index_closest = (const uint32_t*)(D + o_closest); cs.index_many = (const uint32_t*)(D + o_many);
        cs.n_closest = (uint32_t)closest.size(); cs.n_many = (uint32_t)many.size();
        cs.any_body = any_body; cs.any_collider = any_collider; cs.max_body = max_body; cs.max_collider = max_collider;
        cs.any_capsule = is_shape && sp_any_capsule(d.shape, n, false);
        cs.hit_cap = d.hit_cap;
        cs.n = n;
        return AVN_OK;
    }
    avn_status spatial_ray_casters_upload(const avn_spatial_ray_casters* c) override {
        if (!c) { error = "spatial_ray_casters_upload: null argument"; return AVN_ERR_BAD_ARG; }
        const CasterDef d{c->count, c->hit_cap, c->anchor_kind, c->anchor, c->origin, c->direction, c->max_distance, c->max_hits, c->solid, nullptr, nullptr, nullptr,
                          c->enabled, c->mask, c->self_entity, c->excluded_offset, c->excluded};
        return casters_upload(cs_ray, d, false, "spatial_ray_casters_upload");
    }
    avn_status spatial_shape_casters_upload(const avn_spatial_shape_casters* c) override {
        if (!c) { error = "spatial_shape_casters_upload: null argument"; return AVN_ERR_BAD_ARG; }
        const CasterDef d{c->count, c->hit_cap, c->anchor_kind, c->anchor, c->origin, c->direction, c->max_distance, c->max_hits, nullptr, c->shape, c->half_extents,
                          c->shape_rotation, c->enabled, c->mask, c->self_entity, c->excluded_offset, c->excluded};
        return casters_upload(cs_shape, d, true, "spatial_shape_casters_upload");
    }
    // snapshot, re-aim, cast: enqueued on the world's stream, nothing read back
    avn_status spatial_casters_run(uint32_t flags) override {
        cs_ran = false;
        if (flags & ~(uint32_t)AVN_SPATIAL_SKIP_HOST_SHAPES) { error = "spatial_casters_run: flags may only be AVN_SPATIAL_SKIP_HOST_SHAPES"; return AVN_ERR_BAD_ARG; }
        avn_status st = spatial_update();
        if (st != AVN_OK) return st;
        for (const CasterSet* cs : {&cs_ray, &cs_shape}) {
            if (cs->n && ((cs->any_body && cs->max_body >= dw.n_bodies) || (cs->any_collider && cs->max_collider >= bp.n_colliders))) {
                error = "spatial_casters_run: a caster's anchor is outside the current body / collider table (upload the casters again)"; return AVN_ERR_STATE;
            }
        }
        if ((cs_ray.n || cs_shape.n) && (st = sp_check(flags)) != AVN_OK) return st;   // (no casters: the run is the update)
        if (!b_cs_stats.p) {
            ALLOC(b_cs_stats.ensure(4 * sizeof(unsigned long long)));
        }
        unsigned long long* stats = b_cs_stats.as<unsigned long long>();
        HIPCHK(hipMemsetAsync(stats, 0, 4 * sizeof(unsigned long long), stream));
        for (CasterSet* cs : {&cs_ray, &cs_shape}) {
            if (!cs->n) continue;
            const bool is_shape = cs == &cs_shape;
            launch_spatial_reaim<T>(dw, sp, cs->a, stream);
            SQ<T> q = cs->q;
            q.stats = stats;
            q.n = cs->n_closest; q.index = cs->index_closest;
            launch_spatial_casters<T>(sp, q, is_shape ? SPQ_CAST : SPQ_CLOSEST, stream, cs->any_capsule, sp_ccap, sp_tri_table());   // (sp_ccap, sp_ctri: of the update above)
            q.n = cs->n_many; q.index = cs->index_many;
            launch_spatial_casters<T>(sp, q, is_shape ? SPQ_CAST_HITS : SPQ_HITS, stream, cs->any_capsule, sp_ccap, sp_tri_table());
        }
        HIPCHK(hipGetLastError());
        cs_ran = true;
        return AVN_OK;
    }
    avn_status casters_results_check(const char* who) {
        if (!sp_valid || !cs_ran) { error = std::string(who) + ": no avn_spatial_casters_run since the tables or the casters last changed"; return AVN_ERR_STATE; }
        return AVN_OK;
    }
    // waits for the run; its counters become the ones avn_spatial_stats_get reports
    avn_status casters_finish() {
        HIPCHK(hipMemcpyAsync(sp_visits, b_cs_stats.p, sizeof sp_visits, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        if (sp_visits[2]) { error = "spatial casters: traversal stack overflow"; return AVN_ERR_CAPACITY; }
        return AVN_OK;
    }
    avn_status casters_hits_get(const CasterSet& cs, size_t rec, uint32_t flags, void* hits, uint32_t* count, const char* who) {
        if (flags & ~(uint32_t)AVN_SPATIAL_DEVICE_POINTERS) { error = std::string(who) + ": flags may only be AVN_SPATIAL_DEVICE_POINTERS"; return AVN_ERR_BAD_ARG; }
        avn_status st = casters_results_check(who);
        if (st != AVN_OK) return st;
        if (cs.n && (!hits || !count)) { error = std::string(who) + ": null array"; return AVN_ERR_BAD_ARG; }
        const hipMemcpyKind kind = (flags & AVN_SPATIAL_DEVICE_POINTERS) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
        if (cs.n) {
            HIPCHK(hipMemcpyAsync(hits, cs.records, rec * cs.n * cs.hit_cap, kind, stream));
            HIPCHK(hipMemcpyAsync(count, cs.q.count, 4 * (size_t)cs.n, kind, stream));
        }
        return casters_finish();
    }
    avn_status spatial_ray_caster_hits_get(uint32_t flags, const avn_spatial_hits_out* out) override {
        if (!out) { error = "spatial_ray_caster_hits_get: null argument"; return AVN_ERR_BAD_ARG; }
        return casters_hits_get(cs_ray, sizeof(SpatialHit<T>), flags, out->hits, out->count, "spatial_ray_caster_hits_get");
    }
    avn_status spatial_shape_caster_hits_get(uint32_t flags, const avn_spatial_shape_hits_out* out) override {
        if (!out) { error = "spatial_shape_caster_hits_get: null argument"; return AVN_ERR_BAD_ARG; }
        return casters_hits_get(cs_shape, sizeof(SpatialShapeHit<T>), flags, out->hits, out->count, "spatial_shape_caster_hits_get");
    }
    avn_status spatial_caster_poses_get(uint32_t kind, uint32_t flags, const avn_spatial_caster_poses_out* out) override {
        if (!out || kind > AVN_SPATIAL_CASTER_SHAPE || (flags & ~(uint32_t)AVN_SPATIAL_DEVICE_POINTERS)) { error = "spatial_caster_poses_get: bad argument"; return AVN_ERR_BAD_ARG; }
        avn_status st = casters_results_check("spatial_caster_poses_get");
        if (st != AVN_OK) return st;
        const CasterSet& cs = kind == AVN_SPATIAL_CASTER_SHAPE ? cs_shape : cs_ray;
        if (cs.n && (!out->origin || !out->direction || (cs.a.g_rotation && !out->rotation))) { error = "spatial_caster_poses_get: null array"; return AVN_ERR_BAD_ARG; }
        const hipMemcpyKind mk = (flags & AVN_SPATIAL_DEVICE_POINTERS) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
        if (cs.n) {
            HIPCHK(hipMemcpyAsync(out->origin, cs.a.g_origin, 3 * sizeof(T) * cs.n, mk, stream));
            HIPCHK(hipMemcpyAsync(out->direction, cs.a.g_direction, 12 * (size_t)cs.n, mk, stream));
            if (cs.a.g_rotation) HIPCHK(hipMemcpyAsync(out->rotation, cs.a.g_rotation, 4 * sizeof(T) * cs.n, mk, stream));
        }
        return casters_finish();
    }

    avn_status spatial_stats_get(avn_spatial_stats* o) override {
        if (!o) return AVN_ERR_BAD_ARG;
        std::memset(o, 0, sizeof *o);
        o->colliders = sp_valid ? sp.n : 0u;
        o->nodes = sp_valid && sp.n ? 2 * sp.n - 1 : 0u;
        o->host_skipped = sp_valid ? sp_host : 0u;
        o->valid = sp_valid ? 1u : 0u;
        o->nodes_visited = sp_visits[0];
        o->leaves_visited = sp_visits[1];
        return AVN_OK;
    }
