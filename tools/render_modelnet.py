"""ModelNet meshes -> GZIP TFRecords of rendered views, on the device (replaces the reference's off2obj.py ->
obj2png.py -> create_modelnet_tf_record.py chain).

    python tools/render_modelnet.py --src ModelNet40 --split train --out modelnet40_train.tfrecord --views 12 --size 224 [--samples 4] [--shading smooth --light camera --diffuse lambert --specular 0.3]

Walks SRC/<class>/<split>/*.off in sorted order; the label of a shape is the index of its class directory among the
sorted class directories (create_modelnet_tf_record.py's convention).  Meshes are rendered `--batch` at a time with
render.ViewRenderer (uint8, the reference's cameras and shading) and written as tf.Example records of V PNGs that
records.ViewBatcher reads.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def find_shapes(src, split):
    classes = sorted(d for d in os.listdir(src) if os.path.isdir(os.path.join(src, d)))
    shapes = []
    for label, cls in enumerate(classes):
        d = os.path.join(src, cls, split)
        if os.path.isdir(d):
            shapes += [(os.path.join(d, f), label) for f in sorted(os.listdir(d)) if f.lower().endswith(".off")]
    return classes, shapes


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--src", required=True, help="ModelNet root: <class>/<split>/*.off")
    ap.add_argument("--split", default="train")
    ap.add_argument("--out", required=True, help="GZIP TFRecord file to write")
    ap.add_argument("--views", type=int, default=12)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--elevation", type=float, default=30.0)
    ap.add_argument("--fov", type=float, default=0.0)
    ap.add_argument("--samples", type=int, default=1, choices=(1, 2, 4),
                    help="coverage samples per pixel and axis (anti-aliasing inside the rasteriser)")
    ap.add_argument("--shading", default="flat", choices=("flat", "smooth"),
                    help="smooth: Phong reflection on interpolated vertex normals (the look of the published 12-view sets)")
    ap.add_argument("--light", default="world", choices=("world", "camera"),
                    help="camera: a headlight that travels with the view (smooth only)")
    ap.add_argument("--diffuse", default="wrap", choices=("wrap", "lambert"), help="lambert: max(s, 0) (smooth only)")
    ap.add_argument("--specular", type=float, default=0.0, help="weight of the highlight in [0, 1] (smooth only)")
    ap.add_argument("--shininess", type=int, default=16, help="exponent of the highlight: 1, 2, 4, ..., 128")
    ap.add_argument("--two-sided", action="store_true", help="shade both faces alike (inconsistently wound meshes)")
    ap.add_argument("--batch", type=int, default=32, help="meshes per device render")
    ap.add_argument("--encode", default="host", choices=("host", "device"),
                    help="host: copy the pixels back and deflate every view with zlib; device: the views leave the device as "
                         "finished PNG streams (adaptive line filter, colour type 0 for gray views; ViewRenderer.render_png)")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    import torch
    import gvcnn_tf_amd as gv
    from gvcnn_tf_amd import records, render

    classes, shapes = find_shapes(a.src, a.split)
    if not shapes:
        raise SystemExit("no %s/*.off files under %s" % (a.split, a.src))
    dev = torch.device(a.device)
    r = render.ViewRenderer(a.views, a.size, a.size, elevation=a.elevation, fov=a.fov, device=dev,
                            samples=a.samples, shading=a.shading, diffuse=a.diffuse, specular=a.specular,
                            shininess=a.shininess, two_sided=a.two_sided,
                            **({"light": "camera"} if a.light == "camera" else {}))

    def examples():
        for b0 in range(0, len(shapes), a.batch):
            part = shapes[b0:b0 + a.batch]
            meshes = [render.load_off(p) for p, _ in part]
            if a.encode == "device":
                encoded = r.render_png(meshes)
            else:
                views = r.render_uint8(meshes).cpu().numpy()
                encoded = ([records.encode_png(v[i]) for i in range(a.views)] for v in views)
            for (p, label), st, pngs in zip(part, r.status, encoded):
                if st != gv._lib.GV_RENDER_OK:
                    print("warning: %s renders as background (%s)" % (p, render.STATUS.get(int(st), st)),
                          file=sys.stderr)
                yield records.make_example(pngs, label)
    records.write_tfrecords(a.out, examples())
    print("%d shapes of %d classes -> %s" % (len(shapes), len(classes), a.out))


if __name__ == "__main__":
    main()
