#!/usr/bin/env python3
"""Extract the numbers the reference's source text holds for this path into tests/golden/reference_constants.json, and its
two benchmark scene files into tests/golden/reference_scenes/ (what tests/test_reference_constants.py compares against).

    python tools/gen_reference_constants.py REFERENCE_ROOT

Only DATA is extracted, each value by a regular expression over the source text: the material enum's order, the loader's
defaults and clamps, the camera's defaults, mg_ray_tracer's constants, the pack multiplier, whether reflect() is
v - 2 dot(v, n) n.  Nothing of the reference's code is stored.
"""
import json
import re
import shutil
import sys
from pathlib import Path


def number(pattern, source, group=1):
    m = re.search(pattern, source)
    assert m, f"pattern not found in the reference: {pattern}"
    return float(m.group(group).rstrip("fFuU"))


def floats(pattern, source):
    m = re.search(pattern, source)
    assert m, f"pattern not found in the reference: {pattern}"
    return [float(g) for g in m.groups()]


def extract(ref: Path) -> dict:
    common = (ref / "src/common.hpp").read_text()
    scene = (ref / "src/scene.cpp").read_text()
    cam = (ref / "src/camera.hpp").read_text()
    mg = (ref / "src/renderers/mg_ray_tracer.cpp").read_text()
    colour = (ref / "src/colour.hpp").read_text()

    body = re.search(r"enum class material_type\s*:\s*unsigned\s*\{([^}]*)\}", common).group(1)
    clamp = r'"samples_per_pixel",\s*\d+u\),\s*(\d+)u,\s*(\d+)u\)'
    rough = re.search(r'"roughness",\s*type == material_type::dielectric \?\s*([0-9.]+)f\s*:\s*([0-9.]+)f', scene)
    empty = re.search(r"materials\.push_back\(\"\"s,\s*material_type::(\w+),\s*colours::(\w+),\s*([0-9.]+)f,\s*([0-9.]+)f\)", scene)
    sphere = re.search(r'rt::sphere\{\s*deserialize\(tbl,\s*"position",\s*vec3\{\s*([-0-9.]+),\s*([-0-9.]+),\s*([-0-9.]+)\s*\}\),\s*//\s*deserialize\(tbl,\s*"radius",\s*([0-9.]+)f\)', scene)
    box = re.search(r'rt::box\{\s*deserialize\(tbl,\s*"position",\s*vec3\{\s*([-0-9.]+),\s*([-0-9.]+),\s*([-0-9.]+)\s*\}\),\s*//\s*deserialize\(tbl,\s*"extents",\s*vec3\{\s*([0-9.]+)f\s*\}\)', scene)
    return {
        "material_types": [n.strip() for n in body.split(",") if n.strip()],
        "loader": {
            "samples_per_pixel_default": number(r'"samples_per_pixel",\s*(\d+)u\)', scene),
            "max_bounces_default": number(r'"max_bounces",\s*(\d+)u\)', scene),
            "samples_per_pixel_clamp": [number(clamp, scene, 1), number(clamp, scene, 2)],
            "reflectivity_by_type": {k: float(v) for k, v in re.findall(r"case material_type::(\w+):\s*reflectiveness\s*=\s*([0-9.]+)f", scene)},
            "reflectivity_default": number(r"default:\s*reflectiveness\s*=\s*([0-9.]+)f", scene),
            "roughness_dielectric": float(rough.group(1)),
            "roughness_default": float(rough.group(2)),
            "empty_scene_material": {"type": empty.group(1), "colour": empty.group(2), "roughness": float(empty.group(3)), "reflectivity": float(empty.group(4))},
            "sphere_default": [float(g) for g in sphere.groups()],
            "box_default": [float(g) for g in box.groups()],
            "plane_normal_default": floats(r'"normal",\s*vec3\{\s*([-0-9.]+),\s*([-0-9.]+),\s*([-0-9.]+)\s*\}', scene),
            "camera_position_default": floats(r'"position",\s*vec3\{\s*([-0-9.]+),\s*([-0-9.]+),\s*([-0-9.]+)\s*\}\),\s*deserialize\(\*camera', scene),
        },
        "camera": {
            "near": number(r"float near_\s*=\s*([0-9.]+)f", cam),
            "far": number(r"float far_\s*=\s*([0-9.]+)f", cam),
            "vfov_is_pi_over_four": bool(re.search(r"float vfov_\s*=\s*floats::pi_over_four", cam)),
            "position": floats(r"vec3 pos_\s*=\s*\{\s*([-0-9.]+),\s*([-0-9.]+),\s*([-0-9.]+)\s*\}", cam),
        },
        "path": {
            "min_hit_dist": number(r"min_hit_dist\s*=\s*([0-9.]+)f", mg),
            "sky": floats(r"vec3::lerp\(colours::white\.rgb,\s*vec3\{\s*([0-9.]+)f,\s*([0-9.]+)f,\s*([0-9.]+)f\s*\},\s*0\.5f \* \(r\.direction\.y \+ 1\.0f\)\)", mg),
            "pack_multiplier": number(r"vec4\{\s*(255\.[0-9]+)f\s*\}", colour),
            "reflect_is_v_minus_2_dot_v_n_n": bool(re.search(r"return v - 2 \* vec3::dot\(v, n\) \* n;", common)),
        },
    }


def main() -> None:
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ref = Path(sys.argv[1])
    golden = Path(__file__).resolve().parent.parent / "tests" / "golden"
    (golden / "reference_constants.json").write_text(json.dumps(extract(ref), indent=1, sort_keys=True) + "\n")
    (golden / "reference_scenes").mkdir(exist_ok=True)
    for name in ("basic.toml", "dielectric.toml"):
        shutil.copyfile(ref / "scenes" / name, golden / "reference_scenes" / name)
    print(f"wrote {golden / 'reference_constants.json'} and {golden / 'reference_scenes'}/")


if __name__ == "__main__":
    main()
