// avn_spatial.cpp — the extern "C" boundary of include/avian_mi355x_spatial.h over the C++ host world (world/spatial.hpp).
// As in avn_abi.cpp, no exception or HIP error crosses it: every entry point returns avn_status.
#include <new>

#include "avn_world.hpp"

#define SP_GUARD(expr)                                                  \
    do {                                                                \
        if (!w || !w->impl) return AVN_ERR_BAD_ARG;                     \
        try { w->impl->bind(); return w->impl->expr; }                  \
        catch (const std::bad_alloc&) { w->impl->error = "out of host memory"; return AVN_ERR_OOM; } \
        catch (...) { w->impl->error = "unexpected C++ exception"; return AVN_ERR_STATE; }           \
    } while (0)

extern "C" {

AVN_API avn_status avn_spatial_update(avn_world* w) { SP_GUARD(spatial_update()); }
AVN_API avn_status avn_spatial_capsule_colliders_set(avn_world* w, uint32_t enabled) { SP_GUARD(spatial_capsule_colliders_set(enabled)); }
AVN_API avn_status avn_spatial_triangle_colliders_set(avn_world* w, uint32_t enabled) { SP_GUARD(spatial_triangle_colliders_set(enabled)); }
AVN_API avn_status avn_spatial_cast_rays(avn_world* w, const avn_spatial_rays* r, const avn_spatial_hits_out* o) { SP_GUARD(spatial_cast_rays(r, 0u, o)); }
AVN_API avn_status avn_spatial_ray_hits(avn_world* w, const avn_spatial_rays* r, uint32_t max_hits, const avn_spatial_hits_out* o) {
    if (w && w->impl && (max_hits == 0 || max_hits > AVN_SPATIAL_MAX_HITS)) { w->impl->error = "spatial_ray_hits: max_hits must be 1 .. AVN_SPATIAL_MAX_HITS"; return AVN_ERR_BAD_ARG; }
    SP_GUARD(spatial_cast_rays(r, max_hits, o));
}
AVN_API avn_status avn_spatial_point_intersections(avn_world* w, const avn_spatial_points* p, uint32_t cap, const avn_spatial_ids_out* o) { SP_GUARD(spatial_point_intersections(p, cap, o)); }
AVN_API avn_status avn_spatial_aabb_intersections(avn_world* w, const avn_spatial_aabbs* b, uint32_t cap, const avn_spatial_ids_out* o) { SP_GUARD(spatial_aabb_intersections(b, cap, o)); }
AVN_API avn_status avn_spatial_project_points(avn_world* w, const avn_spatial_solid_points* p, const avn_spatial_projections_out* o) { SP_GUARD(spatial_project_points(p, o)); }
AVN_API avn_status avn_spatial_shape_intersections(avn_world* w, const avn_spatial_shapes* s, uint32_t cap, const avn_spatial_ids_out* o) { SP_GUARD(spatial_shape_intersections(s, cap, o)); }
AVN_API avn_status avn_spatial_cast_shapes(avn_world* w, const avn_spatial_shape_casts* c, const avn_spatial_shape_hits_out* o) { SP_GUARD(spatial_cast_shapes(c, 0u, o)); }
AVN_API avn_status avn_spatial_shape_hits(avn_world* w, const avn_spatial_shape_casts* c, uint32_t max_hits, const avn_spatial_shape_hits_out* o) {
    if (w && w->impl && (max_hits == 0 || max_hits > AVN_SPATIAL_MAX_HITS)) { w->impl->error = "spatial_shape_hits: max_hits must be 1 .. AVN_SPATIAL_MAX_HITS"; return AVN_ERR_BAD_ARG; }
    SP_GUARD(spatial_cast_shapes(c, max_hits, o));
}
AVN_API avn_status avn_spatial_shape_contacts(avn_world* w, const avn_spatial_shape_contact_queries* q, uint32_t cap, const avn_spatial_shape_contacts_out* o) { SP_GUARD(spatial_shape_contacts(q, cap, o)); }
AVN_API avn_status avn_spatial_depenetrate(avn_world* w, const avn_spatial_shapes* s, const avn_spatial_depenetration_config* c, const avn_spatial_depenetrations_out* o) { SP_GUARD(spatial_depenetrate(s, c, o)); }
AVN_API avn_status avn_spatial_project_velocities(avn_world* w, const avn_spatial_velocity_projections* p, const avn_spatial_velocities_out* o) { SP_GUARD(spatial_project_velocities(p, o)); }
AVN_API avn_status avn_spatial_cast_moves(avn_world* w, const avn_spatial_moves* m, const avn_spatial_move_hits_out* o) { SP_GUARD(spatial_cast_moves(m, o)); }
AVN_API avn_status avn_spatial_move_and_slide(avn_world* w, const avn_spatial_characters* c, const avn_spatial_move_and_slide_config* cfg, uint32_t hit_cap, const avn_spatial_slides_out* o) {
    SP_GUARD(spatial_move_and_slide(c, cfg, hit_cap, o));
}
AVN_API avn_status avn_spatial_ray_casters_upload(avn_world* w, const avn_spatial_ray_casters* c) { SP_GUARD(spatial_ray_casters_upload(c)); }
AVN_API avn_status avn_spatial_shape_casters_upload(avn_world* w, const avn_spatial_shape_casters* c) { SP_GUARD(spatial_shape_casters_upload(c)); }
AVN_API avn_status avn_spatial_casters_run(avn_world* w, uint32_t flags) { SP_GUARD(spatial_casters_run(flags)); }
AVN_API avn_status avn_spatial_ray_caster_hits_get(avn_world* w, uint32_t flags, const avn_spatial_hits_out* o) { SP_GUARD(spatial_ray_caster_hits_get(flags, o)); }
AVN_API avn_status avn_spatial_shape_caster_hits_get(avn_world* w, uint32_t flags, const avn_spatial_shape_hits_out* o) { SP_GUARD(spatial_shape_caster_hits_get(flags, o)); }
AVN_API avn_status avn_spatial_caster_poses_get(avn_world* w, uint32_t kind, uint32_t flags, const avn_spatial_caster_poses_out* o) { SP_GUARD(spatial_caster_poses_get(kind, flags, o)); }
AVN_API avn_status avn_spatial_stats_get(avn_world* w, avn_spatial_stats* o) { SP_GUARD(spatial_stats_get(o)); }
// include/avian_mi355x_ccd.h (world/ccd.hpp)
AVN_API avn_status avn_swept_ccd_upload(avn_world* w, const avn_swept_ccd* l) { if (w && w->impl) w->impl->touched(); SP_GUARD(swept_ccd_upload(l)); }
AVN_API avn_status avn_swept_ccd_results_get(avn_world* w, avn_swept_ccd_results_out* o) { SP_GUARD(swept_ccd_results_get(o)); }
AVN_API avn_status avn_swept_ccd_non_linear_set(avn_world* w, uint32_t enabled) { SP_GUARD(swept_ccd_non_linear_set(enabled)); }
AVN_API avn_status avn_swept_ccd_capsules_set(avn_world* w, uint32_t enabled) { SP_GUARD(swept_ccd_capsules_set(enabled)); }
AVN_API avn_status avn_swept_ccd_stats_get(avn_world* w, avn_swept_ccd_stats* o) { SP_GUARD(swept_ccd_stats_get(o)); }
// include/avian_mi355x_trimesh.h (world/triangles.hpp)
AVN_API avn_status avn_collider_triangles_upload(avn_world* w, const avn_collider_triangles* t) { if (w && w->impl) w->impl->touched(); SP_GUARD(collider_triangles_upload(t)); }
AVN_API avn_status avn_triangle_manifolds(avn_world* w, const avn_triangle_pairs* q, const avn_query_manifolds_out* o) { SP_GUARD(triangle_manifolds(q, o)); }

}  // extern "C"
