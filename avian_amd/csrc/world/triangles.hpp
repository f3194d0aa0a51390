// world/triangles.hpp -- fragment of the body of `template <class T> struct World` (avn_world.hip includes it inside the class):
// triangle colliders (include/avian_mi355x_trimesh.h) -- the per-collider table BP::col_tri and the batch query avn_triangle_manifolds.
// The table is SLOT-indexed (three Vec4<T> per collider slot, allocated for cap_colliders slots like col_he): a kernel that reads slot s < n_colliders
// reads records 3 s .. 3 s + 2 < 3 cap_colliders, whatever despawn, re-upload or sleeping did to the slot assignment -- there is no second index.
// Every size is col_tri_bytes<T>(count) (avn_kernels.h): the one place where the record size in the world's scalar enters.

    uint32_t tri_count = 0;                  // colliders uploaded with AVN_SHAPE_TRIANGLE (hs_on_colliders_upload counts them)
    std::vector<uint8_t> h_col_shape;        // the kinds of the last avn_colliders_upload (which records of the table are read)
    DevBuf b_col_tri;

    // avn_colliders_upload: the table names the old upload
    void tri_on_colliders_upload(const avn_colliders* c) {
        bp.col_tri = nullptr;
        tri_count = 0;
        h_col_shape.assign(c->shape, c->shape + c->count);
        for (uint32_t i = 0; i < c->count; ++i) tri_count += c->shape[i] == AVN_SHAPE_TRIANGLE;
    }
    // avn_step and the systems, before doing anything: without the table the kernels would read kind 4 as a cuboid with zero half extents
    avn_status tri_need_table() {
        if (tri_count && !bp.col_tri) { error = "the world holds AVN_SHAPE_TRIANGLE colliders and no triangle table (avn_collider_triangles_upload after every avn_colliders_upload)"; return AVN_ERR_STATE; }
        if (tri_count && (halo_on || dsh_on)) { error = "AVN_SHAPE_TRIANGLE colliders: not in a level-2 / sharded world"; return AVN_ERR_STATE; }
        return AVN_OK;
    }
    avn_status collider_triangles_upload(const avn_collider_triangles* t) override {
        if (!t || t->struct_size != sizeof(avn_collider_triangles)) { error = "collider_triangles_upload: struct_size"; return AVN_ERR_BAD_ARG; }
        if (halo_on || dsh_on) { error = "collider_triangles_upload: not in a level-2 / sharded world"; return AVN_ERR_STATE; }
        if (!have_colliders) { error = "collider_triangles_upload: before colliders_upload"; return AVN_ERR_STATE; }
        const uint32_t C = bp.n_colliders;
        if (t->count != C || h_col_shape.size() != C) { error = "collider_triangles_upload: count differs from the last colliders_upload"; return AVN_ERR_BAD_ARG; }
        if (C && !t->vertices) { error = "collider_triangles_upload: null array"; return AVN_ERR_BAD_ARG; }
        if (C > cap_colliders) { error = "collider_triangles_upload: the collider tables are smaller than the count"; return AVN_ERR_STATE; }
        const T* v = (const T*)t->vertices;
        std::vector<V> rec((size_t)3 * C, make4<T>(0, 0, 0, 0));
        for (uint32_t i = 0; i < C; ++i) {
            if (h_col_shape[i] != AVN_SHAPE_TRIANGLE) continue;
            const uint32_t flags = t->edge_flags ? t->edge_flags[i] : (uint32_t)AVN_TRIANGLE_ALL_EDGES;
            if (flags > 7u) { error = "collider_triangles_upload: an edge flag above 7"; return AVN_ERR_BAD_ARG; }
            const T* x = v + 9 * (size_t)i;
            for (int k = 0; k < 9; ++k)
                if (!finite_t(x[k])) { error = "collider_triangles_upload: a vertex that is not finite"; return AVN_ERR_BAD_ARG; }
            const V3<T> a{x[0], x[1], x[2]}, b{x[3], x[4], x[5]}, c{x[6], x[7], x[8]};
            const V3<T> n = na_cross_host(b - a, c - a);
            const T area2 = (n.x * n.x + n.y * n.y) + n.z * n.z;
            if (!(area2 > T(0))) { error = "collider_triangles_upload: a degenerate triangle (collider " + std::to_string(i) + ")"; return AVN_ERR_BAD_ARG; }
            rec[3 * (size_t)i] = make4<T>(a, bits_to_scalar(flags, T(0)));
            rec[3 * (size_t)i + 1] = make4<T>(b, T(0));
            rec[3 * (size_t)i + 2] = make4<T>(c, T(0));
        }
        // (everything is checked: from here on the previous table is replaced)
        sp_valid = false;   // (the spatial-query snapshot was built under the old table)
        HIPCHK(hipStreamSynchronize(stream)); HIPCHK(hipStreamSynchronize(stream_bp));
        if (!tri_count) { bp.col_tri = nullptr; return AVN_OK; }   // (no record would ever be read: a world without a triangle keeps launching what it always has)
        ALLOC(b_col_tri.ensure(col_tri_bytes<T>(cap_colliders)));
        if (b_col_tri.cap < col_tri_bytes<T>(C)) { error = "collider_triangles_upload: the table is smaller than the count"; return AVN_ERR_STATE; }
        HIPCHK(hipMemcpy(b_col_tri.p, rec.data(), col_tri_bytes<T>(C), hipMemcpyHostToDevice));
        bp.col_tri = b_col_tri.as<V>();   // (no captured launch holds BP: the substep graph's kernels take DW only)
        return AVN_OK;
    }
    static V3<T> na_cross_host(V3<T> a, V3<T> b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

    // avn_triangle_manifolds: contact_manifolds (world/contacts.hpp) with the triangles of the rows that hold one
    avn_status triangle_manifolds(const avn_triangle_pairs* p, const avn_query_manifolds_out* o) override {
        if (!p || !o || p->struct_size != sizeof(avn_triangle_pairs)) { error = "triangle_manifolds: struct_size"; return AVN_ERR_BAD_ARG; }
        if (p->count && (!p->shape1 || !p->shape2 || !p->half_extents1 || !p->half_extents2 || !p->position1 || !p->position2 || !p->rotation1 || !p->rotation2 ||
                         !p->prediction_distance)) { error = "triangle_manifolds: null array"; return AVN_ERR_BAD_ARG; }
        const size_t n = p->count;
        bool tri1 = false, tri2 = false;
        for (size_t i = 0; i < n; ++i) {
            const uint8_t k1 = p->shape1[i], k2 = p->shape2[i];
            if (k1 == AVN_SHAPE_HOST || k2 == AVN_SHAPE_HOST || k1 > AVN_SHAPE_TRIANGLE || k2 > AVN_SHAPE_TRIANGLE) { error = "triangle_manifolds: unknown shape"; return AVN_ERR_BAD_ARG; }
            tri1 = tri1 || k1 == AVN_SHAPE_TRIANGLE; tri2 = tri2 || k2 == AVN_SHAPE_TRIANGLE;
            if ((k1 == AVN_SHAPE_TRIANGLE && p->edge_flags1 && p->edge_flags1[i] > 7u) || (k2 == AVN_SHAPE_TRIANGLE && p->edge_flags2 && p->edge_flags2[i] > 7u)) { error = "triangle_manifolds: an edge flag above 7"; return AVN_ERR_BAD_ARG; }
        }
        if ((tri1 && !p->vertices1) || (tri2 && !p->vertices2)) { error = "triangle_manifolds: a triangle without vertices"; return AVN_ERR_BAD_ARG; }
        const size_t Q = AVN_MAX_QUERY_POINTS;
        TriQueryStage<T> ts;
        std::memset(&ts, 0, sizeof ts);
        QueryStage<T>& s = ts.q;
        StagePlan plan(*this);
        SIN(shape1, p->shape1, n); SIN(shape2, p->shape2, n);
        SIN(half_extents1, p->half_extents1, 3 * n); SIN(position1, p->position1, 3 * n); SIN(rotation1, p->rotation1, 4 * n);
        SIN(half_extents2, p->half_extents2, 3 * n); SIN(position2, p->position2, 3 * n); SIN(rotation2, p->rotation2, 4 * n);
        SIN(prediction, p->prediction_distance, n);
        if (tri1) { plan.in((const T*)p->vertices1, 9 * n, &ts.vertices1); plan.in(p->edge_flags1, n, &ts.edge_flags1); }
        if (tri2) { plan.in((const T*)p->vertices2, 9 * n, &ts.vertices2); plan.in(p->edge_flags2, n, &ts.edge_flags2); }
        SOUT(point_count, o->point_count, n); SOUT(normal, o->normal, 3 * n);
        SOUT(anchor1, o->anchor1, 3 * Q * n); SOUT(anchor2, o->anchor2, 3 * Q * n); SOUT(point, o->point, 3 * Q * n);
        SOUT(penetration, o->penetration, Q * n); SOUT(feature_id1, o->feature_id1, Q * n); SOUT(feature_id2, o->feature_id2, Q * n);
        COMMIT(plan);
        launch_triangle_manifolds_query<T>(ts, (uint32_t)n, stream);
        HIPCHK(hipGetLastError());
        FINISH(plan);
        HIPCHK(hipStreamSynchronize(stream));
        return AVN_OK;
    }
