// world/spatial.hpp -- fragment of the body of `template <class T> struct World` (avn_world.hip includes it inside the class):
// SpatialQueryPlugin (spatial_query/mod.rs:190-212) on the device -- include/avian_mi355x_spatial.h.  avn_spatial_update builds the LBVH of
// k_spatial.hip from the poses in HBM; the queries stage their inputs, run one traversal launch and copy the answers back.

    SP<T> sp{};
    DevBuf b_sp_pos, b_sp_rot, b_sp_he, b_sp_info, b_sp_smin, b_sp_smax, b_sp_bmin, b_sp_bmax, b_sp_child, b_sp_parent, b_sp_leaf, b_sp_arr, b_sp_bounds,
        b_sp_keys_a, b_sp_vals_a, b_sp_keys_b, b_sp_vals_b, b_sp_hist, b_sp_block_sums, b_sp_stats,
        b_sp_crec, b_sp_ccount,   // depenetrate's contact records [n * AVN_SPATIAL_MAX_HITS] and counts [n]
        b_sl_pos, b_sl_vel, b_sl_time, b_sl_move, b_sl_pred, b_sl_flags, b_sl_iters, b_sl_hits, b_sl_nplanes, b_sl_planes, b_sl_cfg, b_sl_mh,   // move_and_slide's per-character state
        b_mv_pend, b_mv_pcount;   // cast_move's hand-over: the colliders overlapping each query at its start [n * AVN_SPATIAL_MAX_HITS], their counts [n]
    uint32_t sp_cap = 0;
    bool sp_valid = false;      // a snapshot exists and no table changed since (bodies / colliders / collider transforms uploads and avn_despawn clear it)
    uint32_t sp_host = 0;       // AVN_SHAPE_HOST colliders in the snapshot
    unsigned long long sp_visits[3] = {0, 0, 0};   // last query call: node boxes tested, exact tests, stack overflow

    avn_status sp_grow(uint32_t C) {
        if (sp_cap && C <= sp_cap) return AVN_OK;
        HIPCHK(hipStreamSynchronize(stream));   // (the old buffers may still be read by an update in flight)
        const size_t cc = std::max<size_t>({(size_t)C, (size_t)sp_cap + sp_cap / 2, 64});
        bool moved = false;
        GROW(b_sp_pos, cc, sp.pos); GROW(b_sp_rot, cc, sp.rot); GROW(b_sp_he, cc, sp.he); GROW(b_sp_info, cc, sp.info);
        GROW(b_sp_smin, cc, sp.smin); GROW(b_sp_smax, cc, sp.smax);
        GROW(b_sp_bmin, 2 * cc, sp.bmin); GROW(b_sp_bmax, 2 * cc, sp.bmax); GROW(b_sp_child, cc, sp.child); GROW(b_sp_parent, 2 * cc, sp.parent);
        GROW(b_sp_leaf, cc, sp.leaf_col); GROW(b_sp_arr, cc, sp.arrivals); GROW(b_sp_bounds, 8, sp.bounds);
        GROW(b_sp_keys_a, cc, sp.keys_a); GROW(b_sp_vals_a, cc, sp.vals_a); GROW(b_sp_keys_b, cc, sp.keys_b); GROW(b_sp_vals_b, cc, sp.vals_b);
        GROW(b_sp_hist, (size_t)256 * radix_blocks((uint32_t)cc) + 256, sp.hist);
        GROW(b_sp_block_sums, scan_block_sums_needed(256 * radix_blocks((uint32_t)cc)) + 16, sp.block_sums);
        HIPCHK(hipMemset(b_sp_block_sums.p, 0, b_sp_block_sums.cap));   // the one-launch scan's state: zero once, self-cleaning afterwards (avn_scan.h)
        unsigned long long* dummy_s;
        GROW(b_sp_stats, 4, dummy_s);
        sp_cap = (uint32_t)cc;
        return AVN_OK;
    }

    avn_status spatial_update() override {
        if (!have_bodies || !have_colliders) { error = "spatial_update: before bodies_upload / colliders_upload"; return AVN_ERR_STATE; }
        if (despawn_needs_bodies || despawn_needs_colliders) { error = "spatial_update: avn_despawn is still waiting for avn_bodies_upload / avn_colliders_upload"; return AVN_ERR_STATE; }
        const uint32_t C = bp.n_colliders;
        avn_status st = sp_grow(C);
        if (st != AVN_OK) return st;
        sp.n = C;
        launch_spatial_build<T>(dw, bp, sp, stream);
        HIPCHK(hipGetLastError());
        sp_host = (uint32_t)hs_slots.size();
        sp_valid = true;
        return AVN_OK;
    }

    avn_status sp_check(uint32_t flags) {
        if (!sp_valid) { error = "spatial query: no avn_spatial_update since the tables last changed"; return AVN_ERR_STATE; }
        if (sp_host && !(flags & AVN_SPATIAL_SKIP_HOST_SHAPES)) {
            error = "spatial query: the snapshot holds AVN_SHAPE_HOST colliders, which have no device geometry (AVN_SPATIAL_SKIP_HOST_SHAPES leaves them out)";
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
    template <class U> avn_status sp_in(const void* p, size_t count, bool dev, const U** out) {
        if (!p || count == 0) { *out = nullptr; return AVN_OK; }
        if (dev) { *out = (const U*)p; return AVN_OK; }
        return stage_in<U>(p, count, out);
    }
    template <class U> U* sp_out(void* p, size_t count, bool dev) { return dev ? (U*)p : stage_alloc<U>(count); }
    // bytes the staging arena needs for a call (host pointers: inputs and outputs; always: the excluded list)
    static size_t sp_stage_bytes(bool dev, size_t n, size_t in_bytes, size_t out_bytes, size_t n_excluded) {
        return al(n_excluded * 4) + (dev ? 0 : in_bytes + out_bytes + al(n * 4) * 2) + 4096;
    }
    avn_status sp_run(SQ<T>& q, int kind) {
        q.stats = b_sp_stats.as<unsigned long long>();
        launch_spatial_query<T>(sp, q, kind, stream);
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
        if ((st = stage_reserve(sp_stage_bytes(dev, n, 2 * al(3 * sizeof(T) * n) + al(sizeof(T) * n) + al(n), al(n_rec * sizeof(SpatialHit<T>)), ex.size()))) != AVN_OK) return st;
        SQ<T> q{};
        q.n = n; q.cap = max_hits;
        if ((st = sp_in<T>(r->origin, 3 * (size_t)n, dev, &q.a)) != AVN_OK) return st;
        if ((st = sp_in<T>(r->direction, 3 * (size_t)n, dev, &q.b)) != AVN_OK) return st;
        if ((st = sp_in<T>(r->max_distance, n, dev, &q.max_distance)) != AVN_OK) return st;
        if ((st = sp_in<uint8_t>(r->solid, n, dev, &q.solid)) != AVN_OK) return st;
        if ((st = sp_in<uint32_t>(r->filter.mask, n, dev, &q.mask)) != AVN_OK) return st;
        if ((st = stage_in<uint32_t>(ex.data(), ex.size(), &q.excluded)) != AVN_OK) return st;
        q.n_excluded = (uint32_t)ex.size();
        q.hits = sp_out<SpatialHit<T>>(out->hits, n_rec, dev);
        if (many) q.count = sp_out<uint32_t>(out->count, n, dev);
        if ((st = sp_run(q, many ? SPQ_HITS : SPQ_CLOSEST)) != AVN_OK) return st;
        if (!dev) {
            if ((st = stage_out<SpatialHit<T>>(out->hits, q.hits, n_rec)) != AVN_OK) return st;
            if (many && (st = stage_out<uint32_t>(out->count, q.count, n)) != AVN_OK) return st;
        }
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
        if ((st = stage_reserve(sp_stage_bytes(dev, n, 2 * al(3 * sizeof(T) * n), al(n_ids * 4), ex.size()))) != AVN_OK) return st;
        SQ<T> q{};
        q.n = n; q.cap = cap;
        if ((st = sp_in<T>(a, 3 * (size_t)n, dev, &q.a)) != AVN_OK) return st;
        if (kind == SPQ_AABBS && (st = sp_in<T>(b, 3 * (size_t)n, dev, &q.b)) != AVN_OK) return st;
        if ((st = sp_in<uint32_t>(f.mask, n, dev, &q.mask)) != AVN_OK) return st;
        if ((st = stage_in<uint32_t>(ex.data(), ex.size(), &q.excluded)) != AVN_OK) return st;
        q.n_excluded = (uint32_t)ex.size();
        q.ids = n_ids ? sp_out<uint32_t>(out->collider, n_ids, dev) : nullptr;
        q.count = sp_out<uint32_t>(out->count, n, dev);
        if ((st = sp_run(q, kind)) != AVN_OK) return st;
        if (!dev) {
            if ((st = stage_out<uint32_t>(out->collider, q.ids, n_ids)) != AVN_OK) return st;
            if ((st = stage_out<uint32_t>(out->count, q.count, n)) != AVN_OK) return st;
        }
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
        if ((st = stage_reserve(sp_stage_bytes(dev, n, al(3 * sizeof(T) * n) + al(n), al((size_t)n * sizeof(SpatialProjection<T>)), ex.size()))) != AVN_OK) return st;
        SQ<T> q{};
        q.n = n;
        if ((st = sp_in<T>(p->point, 3 * (size_t)n, dev, &q.a)) != AVN_OK) return st;
        if ((st = sp_in<uint8_t>(p->solid, n, dev, &q.solid)) != AVN_OK) return st;
        if ((st = sp_in<uint32_t>(p->filter.mask, n, dev, &q.mask)) != AVN_OK) return st;
        if ((st = stage_in<uint32_t>(ex.data(), ex.size(), &q.excluded)) != AVN_OK) return st;
        q.n_excluded = (uint32_t)ex.size();
        q.proj = sp_out<SpatialProjection<T>>(out->projection, n, dev);
        if ((st = sp_run(q, SPQ_PROJECT)) != AVN_OK) return st;
        if (!dev && (st = stage_out<SpatialProjection<T>>(out->projection, q.proj, n)) != AVN_OK) return st;
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
        if ((st = stage_reserve(sp_stage_bytes(dev, n, 2 * al(3 * sizeof(T) * n) + al(4 * sizeof(T) * n) + al(n), al(n_ids * 4), ex.size()))) != AVN_OK) return st;
        SQ<T> q{};
        q.n = n; q.cap = cap;
        if ((st = sp_in<uint8_t>(s->shape, n, dev, &q.shape)) != AVN_OK) return st;
        if ((st = sp_in<T>(s->half_extents, 3 * (size_t)n, dev, &q.he)) != AVN_OK) return st;
        if ((st = sp_in<T>(s->position, 3 * (size_t)n, dev, &q.a)) != AVN_OK) return st;
        if ((st = sp_in<T>(s->rotation, 4 * (size_t)n, dev, &q.rot)) != AVN_OK) return st;
        if ((st = sp_in<uint32_t>(s->filter.mask, n, dev, &q.mask)) != AVN_OK) return st;
        if ((st = stage_in<uint32_t>(ex.data(), ex.size(), &q.excluded)) != AVN_OK) return st;
        q.n_excluded = (uint32_t)ex.size();
        q.ids = n_ids ? sp_out<uint32_t>(out->collider, n_ids, dev) : nullptr;
        q.count = sp_out<uint32_t>(out->count, n, dev);
        if ((st = sp_run(q, SPQ_SHAPES)) != AVN_OK) return st;
        if (!dev) {
            if ((st = stage_out<uint32_t>(out->collider, q.ids, n_ids)) != AVN_OK) return st;
            if ((st = stage_out<uint32_t>(out->count, q.count, n)) != AVN_OK) return st;
        }
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
        if ((st = stage_reserve(sp_stage_bytes(dev, n, 3 * al(3 * sizeof(T) * n) + al(4 * sizeof(T) * n) + al(sizeof(T) * n) + al(n), al(n_rec * sizeof(SpatialShapeHit<T>)), ex.size()))) != AVN_OK) return st;
        SQ<T> q{};
        q.n = n; q.cap = max_hits;
        if ((st = sp_in<uint8_t>(s->shape, n, dev, &q.shape)) != AVN_OK) return st;
        if ((st = sp_in<T>(s->half_extents, 3 * (size_t)n, dev, &q.he)) != AVN_OK) return st;
        if ((st = sp_in<T>(s->position, 3 * (size_t)n, dev, &q.a)) != AVN_OK) return st;
        if ((st = sp_in<T>(s->rotation, 4 * (size_t)n, dev, &q.rot)) != AVN_OK) return st;
        if ((st = sp_in<T>(s->direction, 3 * (size_t)n, dev, &q.b)) != AVN_OK) return st;
        if ((st = sp_in<T>(s->max_distance, n, dev, &q.max_distance)) != AVN_OK) return st;
        if ((st = sp_in<uint32_t>(s->filter.mask, n, dev, &q.mask)) != AVN_OK) return st;
        if ((st = stage_in<uint32_t>(ex.data(), ex.size(), &q.excluded)) != AVN_OK) return st;
        q.n_excluded = (uint32_t)ex.size();
        q.cast = sp_out<SpatialShapeHit<T>>(out->hits, n_rec, dev);
        if (many) q.count = sp_out<uint32_t>(out->count, n, dev);
        if ((st = sp_run(q, many ? SPQ_CAST_HITS : SPQ_CAST)) != AVN_OK) return st;
        if (!dev) {
            if ((st = stage_out<SpatialShapeHit<T>>(out->hits, q.cast, n_rec)) != AVN_OK) return st;
            if (many && (st = stage_out<uint32_t>(out->count, q.count, n)) != AVN_OK) return st;
        }
        return sp_finish();
    }
    // the query-shape fields shared by shape_contacts and depenetrate, staged into sc.q (the SPQ_SHAPES fields); stage_reserve is the caller's
    avn_status sp_contact_inputs(SC<T>& sc, uint32_t n, bool dev, const uint8_t* shape, const void* he, const void* pos, const void* rot, const avn_spatial_filter& f,
                                 const std::vector<uint32_t>& ex) {
        avn_status st;
        SQ<T>& q = sc.q;
        q.n = n;
        if ((st = sp_in<uint8_t>(shape, n, dev, &q.shape)) != AVN_OK) return st;
        if ((st = sp_in<T>(he, 3 * (size_t)n, dev, &q.he)) != AVN_OK) return st;
        if ((st = sp_in<T>(pos, 3 * (size_t)n, dev, &q.a)) != AVN_OK) return st;
        if ((st = sp_in<T>(rot, 4 * (size_t)n, dev, &q.rot)) != AVN_OK) return st;
        if ((st = sp_in<uint32_t>(f.mask, n, dev, &q.mask)) != AVN_OK) return st;
        if ((st = stage_in<uint32_t>(ex.data(), ex.size(), &q.excluded)) != AVN_OK) return st;
        q.n_excluded = (uint32_t)ex.size();
        q.stats = b_sp_stats.as<unsigned long long>();
        return AVN_OK;
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
        if ((st = stage_reserve(sp_stage_bytes(dev, n, 2 * al(3 * sizeof(T) * n) + al(4 * sizeof(T) * n) + al(sizeof(T) * n) + al(n), al(n_rec * sizeof(SpatialShapeContact<T>)), ex.size()))) != AVN_OK) return st;
        SC<T> sc{};
        if ((st = sp_contact_inputs(sc, n, dev, s->shape, s->half_extents, s->position, s->rotation, s->filter, ex)) != AVN_OK) return st;
        if ((st = sp_in<T>(s->prediction_distance, n, dev, &sc.prediction)) != AVN_OK) return st;
        sc.q.cap = cap;
        sc.skip_sensors = (s->flags & AVN_SPATIAL_SKIP_SENSORS) ? 1u : 0u;
        sc.pad_unused = 1u;
        sc.rec = n_rec ? sp_out<SpatialShapeContact<T>>(out->contacts, n_rec, dev) : nullptr;
        sc.q.count = sp_out<uint32_t>(out->count, n, dev);
        launch_spatial_contacts<T>(sp, sc, stream);
        HIPCHK(hipGetLastError());
        if (!dev) {
            if ((st = stage_out<SpatialShapeContact<T>>(out->contacts, sc.rec, n_rec)) != AVN_OK) return st;
            if ((st = stage_out<uint32_t>(out->count, sc.q.count, n)) != AVN_OK) return st;
        }
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
        if ((st = stage_reserve(sp_stage_bytes(dev, n, 2 * al(3 * sizeof(T) * n) + al(4 * sizeof(T) * n) + al(n), al((size_t)n * sizeof(SpatialDepenetration<T>)), ex.size()))) != AVN_OK) return st;
        SpatialDepenetration<T>* d_out = sp_out<SpatialDepenetration<T>>(out->depenetration, n, dev);
        if (cfg->iterations == 0) {
            // depenetration disabled: zero vectors, no traversal (every byte of a record is 0)
            if (n) HIPCHK(hipMemsetAsync(d_out, 0, (size_t)n * sizeof(SpatialDepenetration<T>), stream));
            HIPCHK(hipMemsetAsync(b_sp_stats.p, 0, 4 * sizeof(unsigned long long), stream));
        } else {
            bool moved = false;
            SC<T> sc{};
            uint32_t* d_count;
            GROW(b_sp_crec, std::max<size_t>((size_t)n * AVN_SPATIAL_MAX_HITS, 1), sc.rec);
            GROW(b_sp_ccount, std::max<size_t>(n, 1), d_count);
            if ((st = sp_contact_inputs(sc, n, dev, s->shape, s->half_extents, s->position, s->rotation, s->filter, ex)) != AVN_OK) return st;
            sc.q.cap = AVN_SPATIAL_MAX_HITS;
            sc.q.count = d_count;
            sc.prediction = nullptr;
            sc.prediction_all = (T)cfg->skin_width;
            sc.pad_unused = 0u;   // (k_sp_depenetrate reads the first min(count, cap) records only)
            sc.skip_sensors = (s->flags & AVN_SPATIAL_SKIP_SENSORS) ? 1u : 0u;
            launch_spatial_contacts<T>(sp, sc, stream);
            HIPCHK(hipGetLastError());
            SD<T> d{};
            d.n = n; d.rec = sc.rec; d.count = d_count;
            d.skin_width = (T)cfg->skin_width; d.max_error = (T)cfg->max_depenetration_error; d.rejection = (T)cfg->penetration_rejection_threshold;
            d.iterations = cfg->iterations;
            d.out = d_out;
            launch_spatial_depenetrate<T>(d, stream);
            HIPCHK(hipGetLastError());
        }
        if (!dev && (st = stage_out<SpatialDepenetration<T>>(out->depenetration, d_out, n)) != AVN_OK) return st;
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
        avn_status st;
        if ((st = stage_reserve(sp_stage_bytes(dev, n, al(3 * sizeof(T) * n) + al(n_nrm * 4), al(3 * sizeof(T) * n), 0))) != AVN_OK) return st;
        SV<T> v{};
        v.n = n; v.stride = p->stride;
        if ((st = sp_in<T>(p->velocity, 3 * (size_t)n, dev, &v.velocity)) != AVN_OK) return st;
        if ((st = sp_in<float>(p->normals, n_nrm, dev, &v.normals)) != AVN_OK) return st;
        if ((st = sp_in<uint32_t>(p->normal_count, n, dev, &v.count)) != AVN_OK) return st;
        v.out = sp_out<T>(out->velocity, 3 * (size_t)n, dev);
        launch_spatial_project_velocity<T>(v, stream);
        HIPCHK(hipGetLastError());
        if (!dev && (st = stage_out<T>(out->velocity, v.out, 3 * (size_t)n)) != AVN_OK) return st;
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
        if ((st = stage_reserve(sp_stage_bytes(dev, n, 3 * al(3 * sizeof(T) * n) + al(4 * sizeof(T) * n) + al(sizeof(T) * n) + al(n) + al(4 * (size_t)n), al((size_t)n * sizeof(SpatialMoveHit<T>)), ex.size()))) != AVN_OK) return st;
        SC<T> sc{};   // (the shared staging of the query-shape fields)
        if ((st = sp_contact_inputs(sc, n, dev, s->shape, s->half_extents, s->position, s->rotation, s->filter, ex)) != AVN_OK) return st;
        SM<T> m{};
        m.q = sc.q;
        if ((st = sp_in<T>(s->movement, 3 * (size_t)n, dev, &m.movement)) != AVN_OK) return st;
        if ((st = sp_in<T>(s->skin_width, n, dev, &m.skin)) != AVN_OK) return st;
        if ((st = sp_in<uint32_t>(s->self_entity, n, dev, &m.self_entity)) != AVN_OK) return st;
        m.out = sp_out<SpatialMoveHit<T>>(out->hits, n, dev);
        bool moved = false;
        GROW(b_mv_pend, std::max<size_t>((size_t)n * AVN_SPATIAL_MAX_HITS, 1), m.pending);
        GROW(b_mv_pcount, std::max<size_t>(n, 1), m.pending_count);
        launch_spatial_cast_move<T>(sp, m, true, stream);
        HIPCHK(hipGetLastError());
        if (!dev && (st = stage_out<SpatialMoveHit<T>>(out->hits, m.out, n)) != AVN_OK) return st;
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
        if ((st = stage_reserve(sp_stage_bytes(dev, n, 3 * al(3 * sizeof(T) * n) + al(4 * sizeof(T) * n) + al(n) + al(4 * (size_t)n),
                                               al((size_t)n * sizeof(SpatialSlide<T>)) + al(n_hits * sizeof(SpatialSlideHit<T>)), ex.size()))) != AVN_OK) return st;
        SC<T> sc{};
        if ((st = sp_contact_inputs(sc, n, dev, s->shape, s->half_extents, s->position, s->rotation, s->filter, ex)) != AVN_OK) return st;
        SL<T> l{};
        l.n = n; l.hit_cap = hit_cap; l.n_planes = cfg->n_planes; l.max_planes = cfg->max_planes; l.depen_iterations = cfg->depenetration_iterations;
        l.shape = sc.q.shape; l.he = sc.q.he; l.pos_in = sc.q.a; l.rot = sc.q.rot;
        if ((st = sp_in<T>(s->velocity, 3 * (size_t)n, dev, &l.vel_in)) != AVN_OK) return st;
        const uint32_t* self = nullptr;
        if ((st = sp_in<uint32_t>(s->self_entity, n, dev, &self)) != AVN_OK) return st;
        l.out = sp_out<SpatialSlide<T>>(out->slides, n, dev);
        l.hits = n_hits ? sp_out<SpatialSlideHit<T>>(out->hits, n_hits, dev) : nullptr;
        bool moved = false;
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
        auto depenetrate = [&]() {
            if (cfg->depenetration_iterations) { sc.prediction = nullptr; sc.prediction_all = l.skin; launch_spatial_contacts<T>(sp, sc, stream, false); }
            launch_spatial_slide_phase<T>(l, SPL_DEPENETRATE, stream);
        };
        launch_spatial_slide_phase<T>(l, SPL_BEGIN, stream);
        depenetrate();
        for (uint32_t it = 0; it < cfg->move_and_slide_iterations; ++it) {
            l.iteration = it;
            launch_spatial_slide_phase<T>(l, SPL_SWEEP, stream);
            launch_spatial_cast_move<T>(sp, m, false, stream);
            launch_spatial_slide_phase<T>(l, SPL_ADVANCE, stream);
            sc.prediction = l.pred;
            launch_spatial_contacts<T>(sp, sc, stream, false);
            launch_spatial_slide_phase<T>(l, SPL_PLANES, stream);
        }
        depenetrate();
        launch_spatial_slide_phase<T>(l, SPL_END, stream);
        HIPCHK(hipGetLastError());
        if (!dev) {
            if ((st = stage_out<SpatialSlide<T>>(out->slides, l.out, n)) != AVN_OK) return st;
            if ((st = stage_out<SpatialSlideHit<T>>(out->hits, l.hits, n_hits)) != AVN_OK) return st;
        }
        return sp_finish();
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
