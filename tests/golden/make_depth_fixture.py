"""Writes the depth-supervision fixture under tests/golden/colmap_depth/ byte by byte from COLMAP's documented binary model format, as
make_scene_fixtures.py writes its model (nothing here goes through scene_io): one PINHOLE camera of 64 x 48 pixels, two images and
ten 3-D points whose tracks and positions are chosen so that, for image 1, scene_io.view_depth_points keeps some points and drops at
least one for each of its reasons -- left of the image, right of it, above, below, behind the camera -- and one point is named twice
by the image's track entries, one not at all.

    python tests/golden/make_depth_fixture.py
"""
import os
import struct

HERE = os.path.dirname(os.path.abspath(__file__))
D = os.path.join(HERE, "colmap_depth", "sparse", "0")
os.makedirs(D, exist_ok=True)

with open(os.path.join(D, "cameras.bin"), "wb") as f:
    f.write(struct.pack("<Q", 1))
    f.write(struct.pack("<iiQQ", 1, 1, 64, 48))  # PINHOLE: fx, fy, cx, cy
    f.write(struct.pack("<4d", 50.0, 52.0, 32.0, 24.0))

# image 1 looks down +z from z = -4 (R = I, t = (0, 0, 4)); image 2 is turned by 30 degrees about y and shifted
imgs = [
    (1, (1.0, 0.0, 0.0, 0.0), (0.0, 0.0, 4.0), 1, "view_a.png", [(32.0, 24.0, 101), (40.0, 20.0, 102), (1.0, 1.0, -1)]),
    (2, (0.9659258262890683, 0.0, 0.25881904510252074, 0.0), (0.25, -0.125, 5.0), 1, "view_b.png", [(30.0, 22.0, 101)]),
]
with open(os.path.join(D, "images.bin"), "wb") as f:
    f.write(struct.pack("<Q", len(imgs)))
    for iid, q, t, cid, name, pts in imgs:
        f.write(struct.pack("<i4d3di", iid, *q, *t, cid))
        f.write(name.encode() + b"\x00")
        f.write(struct.pack("<Q", len(pts)))
        for x, y, pid in pts:
            f.write(struct.pack("<ddq", x, y, pid))

# (id, xyz, track): in image 1 a point (X, Y, Z) lands at x = 50 X / (Z + 4) + 32, y = 52 Y / (Z + 4) + 24 at depth Z + 4
pts3 = [
    (101, (0.0, 0.0, 0.0), [(1, 0), (2, 0)]),                # the centre, depth 4
    (102, (0.625, -0.25, 1.0), [(1, 1)]),                    # inside
    (103, (-2.5, 1.75, 0.0), [(1, 2), (2, 1)]),              # x = 0.75, y = 46.75: inside, near two edges
    (104, (-2.75, 0.0, 0.0), [(1, 3)]),                      # x = -2.375: left of the image
    (105, (2.6, 0.0, 0.0), [(1, 4)]),                        # x = 64.5: right of it
    (106, (0.0, -2.0, 0.0), [(1, 5), (2, 2)]),               # y = -2: above
    (107, (0.0, 1.9, 0.0), [(1, 6)]),                        # y = 48.7: below
    (108, (0.1, 0.1, -6.0), [(1, 7)]),                       # z = -2: behind the camera (its projection falls inside the image)
    (109, (0.5, 0.5, 2.0), [(1, 8), (1, 9)]),                # named twice by image 1: kept twice
    (110, (0.2, 0.2, 0.5), [(2, 3)]),                        # not in image 1's tracks at all
]
with open(os.path.join(D, "points3D.bin"), "wb") as f:
    f.write(struct.pack("<Q", len(pts3)))
    for pid, xyz, track in pts3:
        f.write(struct.pack("<Q3d3BdQ", pid, *xyz, 128, 128, 128, 0.5, len(track)))
        for iid, idx in track:
            f.write(struct.pack("<ii", iid, idx))
print("wrote", D)
