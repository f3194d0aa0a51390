// world/bodies.hpp -- fragment of the body of `template <class T> struct World` (avn_world.hip includes it inside the class):
// SolverBodyPlugin's component side: avn_bodies_upload / _download, avn_solver_bodies_download.

    // ---- bodies ------------------------------------------------------------------------------------------
    static constexpr uint32_t DUMMY_SLOTS = 2 * AVN_JOINT_TYPE_COUNT;  // joint_damping::<T>: two fresh DUMMY SolverBodies per joint type
    avn_status bodies_upload(const avn_bodies* b) override {
        sp_valid = false;   // (the spatial-query snapshot names the old tables: avn_spatial_update again)
        slp_world_asleep = slp_world_idle = false;
        bodies_prepared_early = false; constraints_prepared_early = false; slot_clear_pending = false;   // (whatever an aborted step left behind: the new bodies are prepared by the next solver front)
        if (!b || (b->count && (!b->position || !b->rotation || !b->linear_velocity || !b->angular_velocity || !b->inv_mass || !b->inv_inertia_local || !b->rb_type))) {
            error = "bodies_upload: null array"; return AVN_ERR_BAD_ARG;
        }
        uint32_t n = b->count;
        bool moved = false;
        // the sharded closed loop's owner table (dsh_owner / b_dsh_owner / dsh_list) is per body and fixed at avn_dshard_enable: k_pg_local_lists reads owner[body]
        if (dsh_on && n != dw.n_bodies) { error = "bodies_upload: another body count inside a sharded closed loop (avn_dshard_enable named an owner per body): avn_dshard_enable(NULL), restart the loop (avn_pipeline_enable(0), uploads, avn_pipeline_enable(1)), avn_dshard_enable with the new owners"; return AVN_ERR_STATE; }
        if (despawn_needs_bodies && n != despawn_expected_bodies) { error = "bodies_upload: after avn_despawn exactly the remaining bodies must be uploaded"; return AVN_ERR_STATE; }
        const bool after_despawn = despawn_needs_bodies;   // (the library has renumbered everything it holds for exactly this upload)
        if (pipe_on && have_bodies && n < dw.n_bodies && !after_despawn) {
            // a despawn renumbers bodies: every contact row, colour mask and handle list of the closed loop names body indices.  Nothing is
            // touched; the host ends the loop (avn_pipeline_enable(0)), uploads the new bodies and colliders and starts it again.
            error = "bodies_upload: fewer bodies than before while the closed loop is on: call avn_despawn for the bodies that leave (or avn_pipeline_enable(0), upload, enable again)";
            return AVN_ERR_STATE;
        }
        if (n + DUMMY_SLOTS > cap_bodies || !have_bodies) {
            HIPCHK(hipStreamSynchronize(stream));
            size_t c = (size_t)std::max<uint32_t>(n + DUMMY_SLOTS, cap_bodies + cap_bodies / 2);  // + the virtual DUMMY bodies of joint_damping
            GROW(b_pos, c, dw.pos, &moved); GROW(b_rot, c, dw.rot, &moved); GROW(b_lvel, c, dw.lvel, &moved); GROW(b_avel, c, dw.avel, &moved); GROW(b_com, c, dw.com, &moved);
            GROW(b_iloc_a, c, dw.iloc_a, &moved); GROW(b_iloc_b, c, dw.iloc_b, &moved); GROW(b_acc_l, c, dw.acc_l, &moved); GROW(b_acc_a, c, dw.acc_a, &moved); GROW(b_bmeta, c, dw.bmeta, &moved);
            GROW(b_sb_vel, 2 * c, dw.sb_lin.p, &moved); dw.sb_ang.p = dw.sb_lin.p + 1;   // Pair2 slots (avn_device.h)
            GROW(b_sb_delta, 2 * c, dw.sb_dp.p, &moved); dw.sb_dq.p = dw.sb_dp.p + 1;
            GROW(b_si, 2 * c, dw.si_a.p, &moved); dw.si_b.p = dw.si_a.p + 1;
            GROW(b_vid_l, c, dw.vid_l, &moved); GROW(b_vid_a, c, dw.vid_a, &moved);
            GROW(b_pre_dp, c, dw.pre_dp, &moved); GROW(b_pre_dq, c, dw.pre_dq, &moved); GROW(b_sb_flags, c, dw.sb_flags, &moved);
            cap_bodies = (uint32_t)c;
            if (pipe_dev) { avn_status sg = pg_bcol_grow(); if (sg != AVN_OK) return sg; }   // bodies spawned inside the closed loop: their colour masks start empty
        }
        if (dw.n_bodies != n) ccd_clear();   // (header: the SweptCcd list names body indices of the old table)
        if (dw.n_bodies != n && dw.lacc_l) { dw.lacc_l = dw.lacc_a = nullptr; graph_valid = false; }   // (header: an upload with another body count drops the local accelerations)
        if (moved || dw.n_bodies != n) graph_valid = false;
        if (have_bodies && n < dw.n_bodies && !after_despawn) {
            // fewer bodies than before: everything that may still index a body >= n is dropped (the host re-uploads it; nothing
            // may gather or schedule out of range meanwhile) -- uploaded manifolds, joints, colliders whose body is gone
            bool bad_m = false, bad_j = false, bad_c = false;
            if (!use_handles) for (size_t i = 0; i < h_m_body1.size() && !bad_m; ++i) bad_m = (uint32_t)h_m_body1[i] >= n || (uint32_t)h_m_body2[i] >= n;
            for (size_t i = 0; i < h_j_body1.size() && !bad_j; ++i) bad_j = (h_j_body1[i] >= 0 && (uint32_t)h_j_body1[i] >= n) || (h_j_body2[i] >= 0 && (uint32_t)h_j_body2[i] >= n);
            for (size_t i = 0; i < h_col_body.size() && !bad_c; ++i) bad_c = h_col_body[i] >= 0 && (uint32_t)h_col_body[i] >= n;
            if (bad_m || (use_handles && dw.n_manifolds)) {
                uint32_t zero[AVN_GRAPH_COLOR_COUNT + 1] = {0};
                dw.n_manifolds = 0; h_m_body1.clear(); h_m_body2.clear();
                set_color_offsets(zero);
                HIPCHK(hipMemcpyAsync(dw.color_offsets, zero, sizeof zero, hipMemcpyHostToDevice, stream));
                island_mode = false; islands_dirty = false;
            }
            if (bad_j) { dw.n_joints = 0; h_j_body1.clear(); h_j_body2.clear(); h_j_damped.clear(); h_j_collision_disabled.clear(); h_j_type.clear(); any_damped = false; }
            // a halo plan (level-2 sharding) names local body indices too: one that reaches past the new count is dropped with the rest
            bool bad_h = false;
            for (int32_t b : halo.send) bad_h = bad_h || (uint32_t)b >= n;
            for (int32_t b : halo.recv) bad_h = bad_h || (uint32_t)b >= n;
            if (bad_h) { halo = HaloPlan(); halo_on = false; }
            if (bad_c) { bp.n_colliders = 0; bp.n_intervals = 0; have_colliders = false; slot_entity.clear(); entity_slot.clear(); h_col_body.clear(); }
        }
        dw.n_bodies = n;
        BodyStage<T> s;
        std::memset(&s, 0, sizeof s);
        StagePlan plan(*this);
        SIN(position, b->position, 3 * (size_t)n); SIN(rotation, b->rotation, 4 * (size_t)n);
        SIN(linear_velocity, b->linear_velocity, 3 * (size_t)n); SIN(angular_velocity, b->angular_velocity, 3 * (size_t)n);
        SIN(inv_mass, b->inv_mass, n); SIN(inv_inertia_local, b->inv_inertia_local, 6 * (size_t)n);
        SIN(center_of_mass, b->center_of_mass, 3 * (size_t)n); SIN(linear_damping, b->linear_damping, n);
        SIN(angular_damping, b->angular_damping, n); SIN(gravity_scale, b->gravity_scale, n);
        SIN(accel_linear, b->accel_linear, 3 * (size_t)n); SIN(accel_angular, b->accel_angular, 3 * (size_t)n);
        SIN(max_linear_speed, b->max_linear_speed, n); SIN(max_angular_speed, b->max_angular_speed, n);
        SIN(rb_type, b->rb_type, n); SIN(locked_axes, b->locked_axes, n); SIN(body_flags, b->body_flags, n);
        SIN(dominance, b->dominance, n);
        COMMIT(plan);
        launch_pack_bodies<T>(dw, s, stream);
        HIPCHK(hipGetLastError());
        // host copy of "has SolverBody" for the joint schedules
        h_body_has_sb.resize(n); h_rb_type.resize(n); h_body_flags.resize(n);
        std::vector<uint32_t> asleep;
        for (uint32_t i = 0; i < n; ++i) {
            uint8_t fl = b->body_flags ? b->body_flags[i] : 0;
            h_rb_type[i] = b->rb_type[i];
            if (slp_on) {   // the Sleeping component is the island manager's (SleepIslands / WakeIslands), not the uploader's
                if (b->rb_type[i] != AVN_RB_STATIC && !(fl & AVN_BODY_DISABLED) && !isl.body_has_node(i)) { avn_status si = isl.body_add(i); if (si != AVN_OK) { error = isl.error; return si; } }
                if (isl.body_has_node(i) && isl.body_sleeps(i)) { fl |= AVN_BODY_SLEEPING; asleep.push_back(i); } else fl &= (uint8_t)~AVN_BODY_SLEEPING;
            }
            h_body_flags[i] = fl;
            h_body_has_sb[i] = b->rb_type[i] != AVN_RB_STATIC && !(fl & (AVN_BODY_SLEEPING | AVN_BODY_DISABLED));
        }
        if (slp_on) {
            // (the packed flags are the uploader's: put the manager's Sleeping flags back, clear the others)
            std::vector<uint32_t> awake_list;
            for (uint32_t i = 0; i < n; ++i) if (!(h_body_flags[i] & AVN_BODY_SLEEPING) && b->body_flags && (b->body_flags[i] & AVN_BODY_SLEEPING)) awake_list.push_back(i);
            HIPCHK(hipStreamSynchronize(stream));
            const uint32_t *d1 = nullptr, *d2 = nullptr;
            StagePlan plan2(*this);
            plan2.in(asleep.data(), asleep.size(), &d1); plan2.in(awake_list.data(), awake_list.size(), &d2);
            COMMIT(plan2);
            avn_status s2;
            launch_bodies_set_sleeping<T>(dw, d1, (uint32_t)asleep.size(), 1u, nullptr, stream);
            launch_bodies_set_sleeping<T>(dw, d2, (uint32_t)awake_list.size(), 0u, nullptr, stream);
            if ((s2 = slp_grow_bodies(n)) != AVN_OK) return s2;   // spawned bodies: SleepTimer 0, the world's thresholds
        }
        joint_schedule_dirty = true;
        incidence_dirty = true;
        have_bodies = true;
        despawn_needs_bodies = false;
        if (dsh_on) { avn_status sd = dsh_apply_flags(); if (sd != AVN_OK) return sd; }   // (the pack wrote the uploader's flags: AVN_BODY_FOREIGN and the host's SolverBody mirror again)
        HIPCHK(hipStreamSynchronize(stream));  // host arrays are only borrowed for the call
        return AVN_OK;
    }
    // AccumulatedLocalAcceleration (forces/mod.rs:661-673), consumed by apply_local_acceleration in front of integrate_velocities in every substep
    // (forces/plugin.rs:207-241): avn_body_ops.h integrate_velocities_one
    avn_status local_accelerations_upload(uint32_t count, const void* linear, const void* angular) override {
        if (count == 0 || (!linear && !angular)) {
            if (dw.lacc_l) { dw.lacc_l = dw.lacc_a = nullptr; graph_valid = false; }
            return AVN_OK;
        }
        if (!have_bodies || count != dw.n_bodies) { error = "local_accelerations_upload: count differs from the last bodies_upload"; return AVN_ERR_BAD_ARG; }
        if (despawn_needs_bodies) { error = "local_accelerations_upload: avn_despawn removed bodies: upload the remaining bodies (avn_bodies_upload) first"; return AVN_ERR_STATE; }
        slp_world_asleep = slp_world_idle = false;
        Vec4<T>*dl = nullptr, *da = nullptr;
        HIPCHK(hipStreamSynchronize(stream));
        GROW(b_lacc_l, (size_t)cap_bodies, dl); GROW(b_lacc_a, (size_t)cap_bodies, da);
        const T *sl = nullptr, *sa = nullptr;
        StagePlan plan(*this);
        plan.in(linear, 3 * (size_t)count, &sl); plan.in(angular, 3 * (size_t)count, &sa);
        COMMIT(plan);
        launch_pack_local_accelerations<T>(dl, da, sl, sa, count, stream);
        HIPCHK(hipGetLastError());
        if (dw.lacc_l != dl || dw.lacc_a != da) { dw.lacc_l = dl; dw.lacc_a = da; graph_valid = false; }
        HIPCHK(hipStreamSynchronize(stream));  // host arrays are only borrowed for the call
        return AVN_OK;
    }
    avn_status bodies_download(const avn_bodies_out* o) override {
        if (!o) return AVN_ERR_BAD_ARG;
        size_t n = dw.n_bodies;
        T *p, *r, *l, *a;
        StagePlan plan(*this);
        plan.out(o->position, 3 * n, &p); plan.out(o->rotation, 4 * n, &r);
        plan.out(o->linear_velocity, 3 * n, &l); plan.out(o->angular_velocity, 3 * n, &a);
        COMMIT(plan);
        launch_unpack_bodies<T>(dw, p, r, l, a, stream);
        HIPCHK(hipGetLastError());
        FINISH(plan);
        HIPCHK(hipStreamSynchronize(stream));
        return AVN_OK;
    }
    avn_status solver_bodies_download(const avn_solver_bodies_out* o) override {
        if (!o) return AVN_ERR_BAD_ARG;
        size_t n = dw.n_bodies;
        SolverBodiesStage<T> s;
        StagePlan plan(*this);
        SOUT(linear_velocity, o->linear_velocity, 3 * n); SOUT(angular_velocity, o->angular_velocity, 3 * n);
        SOUT(delta_position, o->delta_position, 3 * n); SOUT(delta_rotation, o->delta_rotation, 4 * n);
        SOUT(flags, o->flags, n); SOUT(inv_mass, o->inv_mass, n); SOUT(inv_inertia_world, o->inv_inertia_world, 6 * n);
        SOUT(dominance, o->dominance, n); SOUT(linear_increment, o->linear_increment, 3 * n);
        SOUT(angular_increment, o->angular_increment, 3 * n); SOUT(linear_damping_rhs, o->linear_damping_rhs, n);
        SOUT(angular_damping_rhs, o->angular_damping_rhs, n);
        COMMIT(plan);
        launch_unpack_solver_bodies<T>(dw, s, stream);
        HIPCHK(hipGetLastError());
        FINISH(plan);
        HIPCHK(hipStreamSynchronize(stream));
        return AVN_OK;
    }

