#!/usr/bin/env python3
"""Extract the visual geometry DATA of the reference's URDF into urdf_visuals.json.

Run where a checkout of the reference project is at hand:
    python tests/golden/make_urdf_visuals.py REFERENCE_ROOT | FILE.urdf [OUT.json]
Only numbers and names are copied (every <material>'s rgba; per <visual> its link, origin xyz / rpy as written, geometry
and material name); no reference source text.  OUT.json defaults to urdf_visuals.json next to this script.
"""
import json
import os
import sys
import xml.etree.ElementTree as ET


def floats(text, default):
    return [float(x) for x in text.split()] if text else list(default)


def extract(urdf: str) -> dict:
    root = ET.parse(urdf).getroot()
    materials = {m.get("name"): floats(m.find("color").get("rgba"), ()) for m in root.findall("material")}
    visuals = []
    for link in root.findall("link"):
        for v in link.findall("visual"):
            o = v.find("origin")
            (shape,) = list(v.find("geometry"))
            if shape.tag == "box":
                geom = {"type": "box", "size": floats(shape.get("size"), ())}
            elif shape.tag == "cylinder":
                geom = {"type": "cylinder", "radius": float(shape.get("radius")), "length": float(shape.get("length"))}
            elif shape.tag == "sphere":
                geom = {"type": "sphere", "radius": float(shape.get("radius"))}
            else:
                raise ValueError(f"{link.get('name')}: unsupported visual geometry {shape.tag}")
            m = v.find("material")
            visuals.append({
                "link": link.get("name"),
                "xyz": floats(o.get("xyz") if o is not None else None, (0, 0, 0)),
                # the rpy text as written (1.5708 is not pi/2): kept as strings so the values survive exactly
                "rpy": (o.get("rpy") if o is not None and o.get("rpy") else "0 0 0").split(),
                "geometry": geom,
                "material": m.get("name") if m is not None else None,
            })
    return {"source": "xdralex/pioneer pioneer/envs/pioneer/assets/pioneer_knm_6dof.urdf (numbers only)",
            "materials": materials, "visuals": visuals}


def main():
    if len(sys.argv) not in (2, 3):
        sys.exit(__doc__)
    ref = sys.argv[1]
    urdf = ref if ref.endswith(".urdf") else os.path.join(ref, "pioneer/envs/pioneer/assets/pioneer_knm_6dof.urdf")
    dst = sys.argv[2] if len(sys.argv) == 3 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "urdf_visuals.json")
    out = extract(urdf)
    with open(dst, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {dst}: {len(out['materials'])} materials, {len(out['visuals'])} visuals")


if __name__ == "__main__":
    main()
