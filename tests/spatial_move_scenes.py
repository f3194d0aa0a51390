"""Scenes and characters shared by the move-and-slide tests (tests/test_spatial_moves_cpu.py chooses the seeds and asserts the populations on the
CPU; tests/test_gpu_spatial_moves.py runs the same scenes on the device)."""
import numpy as np

from helpers import F, random_unit_quats
import spatial_query_reference as R
import spatial_scenes as SC

I = [0.0, 0.0, 0.0, 1.0]
BALL, CUBOID = R.SHAPE_BALL, R.SHAPE_CUBOID
SELF_ENTITY = 900
# MoveAndSlideConfig for the random scenes: a rejection threshold small enough that a character sunk deep into the floor is left there by the
# depenetration, so its first cast starts overlapping
CFG = dict(delta_time=0.25, skin_width=0.05, max_depenetration_error=1e-4, penetration_rejection_threshold=0.3, depenetration_iterations=16,
           move_and_slide_iterations=4, max_planes=20, plane_similarity_dot_threshold=0.999)


def room(centre=(0.0, 0.0, 0.0)):
    """Twelve colliders, one per static body: a floor whose top is y = 0, four walls, a ramp rotated about z, a ball pillar, a step, a crate, a
    second ball, one sensor, and one ball that is some character's own collider (entity SELF_ENTITY).  Returns (bodies, colliders, sensor flags)."""
    c, s = np.cos(np.radians(20) / 2), np.sin(np.radians(20) / 2)
    items = [  # (shape, half extents, position, rotation, sensor)
        (CUBOID, [8, 0.5, 8], [0, -0.5, 0], I, 0),
        (CUBOID, [0.5, 2, 6.5], [6.5, 2, 0], I, 0), (CUBOID, [0.5, 2, 6.5], [-6.5, 2, 0], I, 0),
        (CUBOID, [6.5, 2, 0.5], [0, 2, 6.5], I, 0), (CUBOID, [6.5, 2, 0.5], [0, 2, -6.5], I, 0),
        (CUBOID, [2, 0.25, 1.5], [3, 0.5, -3], [0, 0, s, c], 0),
        (BALL, [1, 0, 0], [2, 0.5, 2.5], I, 0),
        (CUBOID, [1, 0.25, 1], [-3, 0.25, -2], I, 0),
        (CUBOID, [0.5, 0.5, 0.5], [-2.5, 0.5, 3], [0, np.sin(0.3), 0, np.cos(0.3)], 0),
        (BALL, [0.5, 0, 0], [-4.5, 0.5, 0.5], I, 0),
        (CUBOID, [1, 1, 1], [0, 1, 0], I, 1),
        (BALL, [0.4, 0, 0], [1.5, 0.45, -1], I, 0),
    ]
    n = len(items)
    cols = dict(entity_index=np.array([100 + k for k in range(n - 1)] + [SELF_ENTITY], np.uint32), body=np.arange(n, dtype=np.int32),
                shape=np.array([i[0] for i in items], np.uint8), half_extents=np.array([i[1] for i in items], float),
                memberships=np.array([1] * 8 + [2, 2, 1, 1], np.uint32), collider_flags=np.array([F.COLLIDER_SENSOR if i[4] else 0 for i in items], np.uint8))
    pos = np.array([i[2] for i in items], float) + np.asarray(centre, float)
    return SC.bodies_of(pos, np.array([i[3] for i in items], float)), cols, np.array([i[4] for i in items], np.uint8)


def characters(seed, n=100, centre=(0.0, 0.0, 0.0)):
    """n characters of both kinds in the room, in six groups by index % 6: 0 high in the air and slow (never hit), 1 above the floor moving
    straight down (one plane), 2 near a corner moving into it (two planes and more), 3 sunk into the floor moving up (overlapping and
    leaving), 4 sunk into the floor moving down (overlapping and blocked), 5 anywhere at random, the first of them on top of the SELF_ENTITY ball
    with that entity as its own, the second a ball whose centre is inside the floor.  Returns (shape, half extents, position, rotation, velocity, self_entity)."""
    rng = np.random.default_rng(seed)
    g = np.arange(n) % 6
    shape = (rng.random(n) < 0.5).astype(np.uint8)
    he = rng.uniform(0.2, 0.5, (n, 3))
    rot = random_unit_quats(rng, n)
    rot[g == 1] = I; rot[g == 3] = I; rot[g == 4] = I
    rot[rng.random(n) < 0.2] = I
    pos = np.c_[rng.uniform(-5, 5, n), rng.uniform(0.2, 3.0, n), rng.uniform(-5, 5, n)]
    vel = rng.normal(size=(n, 3)) * 6
    k = g == 0
    pos[k, 1] = rng.uniform(6, 8, k.sum()); vel[k] = rng.normal(size=(k.sum(), 3)) * 0.5
    k = g == 1
    pos[k] = np.c_[rng.uniform(-5.5, -3.5, k.sum()), he[k, 1] * (shape[k] == CUBOID) + he[k, 0] * (shape[k] == BALL) + rng.uniform(0.2, 0.6, k.sum()), rng.uniform(3, 5, k.sum())]
    vel[k] = np.c_[np.zeros(k.sum()), -rng.uniform(4, 8, k.sum()), np.zeros(k.sum())]
    k = g == 2
    pos[k] = np.c_[rng.uniform(4.5, 5.2, k.sum()), rng.uniform(0.7, 1.0, k.sum()), rng.uniform(4.5, 5.2, k.sum())]
    vel[k] = np.c_[rng.uniform(4, 8, k.sum()), -rng.uniform(4, 8, k.sum()), rng.uniform(4, 8, k.sum())]
    for grp, sign in ((3, 1.0), (4, -1.0)):
        k = g == grp
        pos[k] = np.c_[rng.uniform(-5.5, -3.5, k.sum()), rng.uniform(0.05, 0.15, k.sum()), rng.uniform(-5.5, -3.5, k.sum())]
        he[k] = rng.uniform(0.45, 0.5, (k.sum(), 3))
        vel[k] = np.c_[rng.normal(size=k.sum()), sign * rng.uniform(3, 6, k.sum()), rng.normal(size=k.sum())]
    self_entity = np.full(n, R.MISS, np.uint32)
    self_entity[rng.random(n) < 0.3] = 105      # (someone else's entity: that collider is simply invisible to these characters)
    shape[5] = BALL; he[5] = [0.4, 0, 0]; pos[5] = [1.5, 0.45, -1]; vel[5] = [0, -4, 1]; self_entity[5] = SELF_ENTITY
    shape[11] = BALL; he[11] = [0.45, 0, 0]; pos[11] = [-1, -0.2, 5]; vel[11] = [1, -3, 0]      # its centre inside the floor: an overlap without a contact
    return shape, he, pos + np.asarray(centre, float), rot, vel, self_entity


def moves(seed, n=100, centre=(0.0, 0.0, 0.0)):
    """cast_moves queries over the room: the characters above with movement = velocity * 0.25, skin widths 0 .. 0.1 (some exactly 0), a few
    zero movements."""
    shape, he, pos, rot, vel, self_entity = characters(seed, n, centre)
    rng = np.random.default_rng(seed + 1000)
    movement = vel * 0.25
    movement[rng.random(n) < 0.05] = 0.0
    skin = rng.uniform(0, 0.1, n)
    skin[rng.random(n) < 0.15] = 0.0
    return shape, he, pos, rot, movement, skin, self_entity
