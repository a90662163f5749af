"""Textured mesh export (nerf/mesh.py export_mesh with a texture) stage by stage
on a trainer built as tests/test_mesh.py builds it (17 native steps on random
embeddings):
    python tools/mesh_case.py [--resolution 128] [--texture_size 2048] [--raster-ref]
--texture_size -1 picks the automatic size.  GPU stages are timed with HIP
events, host stages with the wall clock; --raster-ref also runs the f64 numpy
oracle of tests/test_mesh_texture_host.py on the same atlas (the only other
rasteriser there is) and checks the face ids against it."""
import argparse
import os
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "single-stable-dreamfusion_amd"), str(ROOT / "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


class Stages:
    def __init__(self):
        self.rows = []

    def gpu(self, name, fn):
        e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        torch.cuda.synchronize()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        self.rows.append((name, "hip events", e0.elapsed_time(e1)))
        return out

    def host(self, name, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        self.rows.append((name, "wall clock", (time.perf_counter() - t0) * 1e3))
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=128)
    ap.add_argument("--texture_size", type=int, default=2048, help="-1: automatic")
    ap.add_argument("--raster-ref", action="store_true",
                    help="time and compare the f64 numpy rasteriser on the same atlas")
    ap.add_argument("--out", default="", help="directory for the files (default: temporary)")
    args = ap.parse_args()
    import bench
    import _texture
    from nerf import mesh

    trainer, data = bench.make_trainer(64, 3, 0, 1, True, graph=True)
    with torch.no_grad():
        trainer.model.encoder.embeddings.uniform_(-0.5, 0.5)
    for i in range(17):
        trainer.train_iteration(data.collate([i % 4]))
    model = trainer.model
    dev = model.density_bitfield.device
    res = args.resolution
    size = None if args.texture_size < 0 else args.texture_size
    st = Stages()
    with torch.no_grad():
        # load the code objects of every timed kernel before the timed stages
        wvt, wft, wh, ww = mesh.grid_atlas(2, 16)
        wv = np.eye(3, dtype=np.float32)
        wf = np.array([[0, 1, 2]] * 2, np.int32)
        _, wxyz, wmask = mesh.rasterize_uv(wvt, wft, wv, wf, wh, ww)
        mesh.bake_texture(model, wxyz, wmask)
        thresh = min(float(model.mean_density), float(model.density_thresh))
        sig = st.gpu("lattice query", lambda: mesh.query_lattice(model.density, res, 128, dev))
        verts, faces = st.host("isosurface", lambda: mesh.isosurface(sig, thresh))
        verts = (verts / (res - 1.0) * 2 - 1).astype(np.float32)
        faces = faces.astype(np.int32)
        if len(faces) == 0:
            print("empty isosurface: nothing to bake")
            return
        vt, ft, H, W = st.host("atlas", lambda: mesh.grid_atlas(len(faces), size))
        _, xyz, mask = st.gpu("raster", lambda: mesh.rasterize_uv(vt, ft, verts, faces, H, W))
        img = st.gpu("field query", lambda: mesh.query_texels(model, xyz, mask))
        img, _ = st.gpu("dilate", lambda: _texture.texture_dilate(img, mask.to(torch.uint8), 3))
        tmp = None if args.out else tempfile.TemporaryDirectory()
        out = args.out or tmp.name
        os.makedirs(out, exist_ok=True)

        def write():
            mesh.write_png(os.path.join(out, "albedo.png"), img.cpu().numpy())
            mesh.write_mtl(os.path.join(out, "mesh.mtl"), "albedo.png")
            mesh.write_obj_textured(os.path.join(out, "mesh.obj"), verts, faces, vt, ft, "mesh.mtl")

        st.host("file writes", write)
    covered = int(mask.sum())
    print(f"resolution {res}: {len(verts)} vertices, {len(faces)} faces; texture {H} x {W}, "
          f"{covered} covered texels ({100.0 * covered / (H * W):.1f} %)")
    for name, clock, ms in st.rows:
        print(f"  {name:<14s} {ms:10.2f} ms  ({clock})")
    # the two raster kernels alone, operands already on the device
    vt_d, ft_d = torch.from_numpy(vt).to(dev), torch.from_numpy(ft).to(dev)
    v_d, f_d = torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev)
    for what, fn in (("dfhip_raster_uv_faces", lambda: _texture.raster_uv_faces(vt_d, ft_d, H, W)),
                     ("dfhip_raster_uv_interp",
                      lambda: _texture.raster_uv_interp(vt_d, ft_d, v_d, f_d, fid, H, W))):
        def reps(fn=fn):
            for _ in range(10):
                out = fn()
            return out
        out = st.gpu(what, reps)
        if what == "dfhip_raster_uv_faces":
            fid = out
        print(f"  {what} alone: {st.rows[-1][2] / 10:.3f} ms (mean of 10, output allocation "
              "included)")
    faces_ms = st.rows[-2][2] / 10
    if args.raster_ref:
        from test_mesh_texture_host import raster_ref
        t0 = time.perf_counter()
        want = raster_ref(vt, ft, H, W)
        ref_ms = (time.perf_counter() - t0) * 1e3
        same = np.array_equal(fid.cpu().numpy().reshape(H, W), want)
        print(f"  raster_ref (numpy f64, host) {ref_ms:.1f} ms against dfhip_raster_uv_faces "
              f"{faces_ms:.3f} ms; face ids {'equal' if same else 'DIFFER'}")
        if not same:
            sys.exit(1)


if __name__ == "__main__":
    main()
