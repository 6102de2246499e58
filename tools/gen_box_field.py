#!/usr/bin/env python3
"""Writes tests/golden/scenes/box_field.toml: about 300 boxes over a ground plane, the scene of RT_HIP_FLAG_BOX_BVH's headless test
(more boxes than the linear box builds trace: rt_headless --boxes refuses it, --boxes --box-bvh renders it).

    python tools/gen_box_field.py > tests/golden/scenes/box_field.toml

A 20 x 15 block world: columns of pseudo-random height on a jittered grid, a few floating slabs, every fourth block metal and every
ninth glass.  Deterministic (its own small generator, no library's): the same file on every machine."""

HEADER = """# tests/golden/scenes/box_field.toml — this project's own scene for RT_HIP_FLAG_BOX_BVH (DESIGN.md §3.10): 304 boxes over the ground
# plane and one sphere — more boxes than the linear box builds trace (256).  Written by tools/gen_box_field.py; box extents are half sizes.

samples_per_pixel = 16
max_bounces = 6

camera = { position = [0.4, 3.2, 9.5], direction = [0, -0.35, -1] }

materials = [
    { type = 'lambert',    albedo = [0.5, 0.55, 0.5] },
    { type = 'lambert',    albedo = [0.8, 0.35, 0.25] },
    { type = 'metal',      albedo = [0.9, 0.85, 0.7], roughness = 0.15 },
    { type = 'dielectric', albedo = [0.9, 0.95, 1.0] },
    { type = 'lambert',    albedo = [0.25, 0.45, 0.8] },
]

planes = [
    { material = 0 }
]

spheres = [
    { material = 2, position = [0.3, 2.4, 2.5], radius = 0.6 },
]

boxes = ["""


def main():
    state = 2463534242

    def draw():
        nonlocal state
        state ^= (state << 13) & 0xFFFFFFFF
        state ^= state >> 17
        state ^= (state << 5) & 0xFFFFFFFF
        return (state & 0xFFFF) / 65536.0

    print(HEADER)
    count = 0
    for row in range(15):
        for column in range(20):
            x = (column - 9.5) * 0.8 + (draw() - 0.5) * 0.2
            z = 3.0 - row * 0.8 + (draw() - 0.5) * 0.2
            half = 0.2 + 0.15 * draw()
            height = 0.15 + 0.9 * draw() * draw()
            material = 2 if count % 4 == 3 else (3 if count % 9 == 4 else (1 if count % 2 else 4))
            print(f"    {{ material = {material}, position = [{x:.3f}, {height:.3f}, {z:.3f}], extents = [{half:.3f}, {height:.3f}, {half:.3f}] }},")
            count += 1
    for k in range(4):  # floating slabs
        print(f"    {{ material = {1 + k % 2 * 3}, position = [{-4.5 + 3.0 * k:.3f}, {2.2 + 0.3 * k:.3f}, {-2.0 - k:.3f}], extents = [0.900, 0.080, 0.600] }},")
        count += 1
    print("]")
    assert count == 304


if __name__ == "__main__":
    main()
