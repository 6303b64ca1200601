"""Images in, meshes out: inference with a trained scene network, without a dataset tree.

``Reconstructor(model)`` wraps a ``SceneNetTrainer`` (moved to ``.cuda().eval()``);
``Reconstructor.from_checkpoint(path, inf_res=None, scale_factor=None, skip_unet=None, block=None)`` builds the trainer from
the checkpoint's hyper-parameters, with the overrides ``run_scene_net_test`` applies (None keeps the checkpoint's value).

``reconstruct(images, flip=False)``: a path, a PIL image, a uint8 (H, W, 3) array or tensor, or a list of those.  Any other
Pillow mode is converted with ``.convert("RGB")`` on the host.  Equal-sized images run as one batch.  Under ``no_grad``:
ops.rgb_preprocess (the dataset's transform on the device: SquarePad + Pillow's bilinear resize when the model was trained
with resize_input, the flip in front of it, the normalisation) -> UNet -> depth head -> project.depthmap_to_gridspace
(normalize=True) -> project() -> per view the IF-Net lattice on ``model.dims`` at ``res_increase = inf_res`` and marching
cubes (ifnet.implicit_to_vertices; `block` as in implicit_to_mesh).  The depth and voxel stages are the trainer's own
(``SceneNetTrainer._predict_depth`` / ``_voxels_from_depth``), so the tensors are the ones ``forward`` computes; the IF-Net
is never queried on training points and no batch dictionary exists.  One input gives one ``Reconstruction``, a list a list.

``reconstruct_depth(depth)``: the same from a (B, 240, 320) depth tensor (device tensor or numpy array) or from the path
of a distance ``.exr`` (channel R, then FromDistanceToDepth): what a ``skip_unet`` model uses.

``Reconstruction``: `depth` (240, 320), `point_cloud` (76800, 3, normalised grid space), `voxel_occupancy` (1, *dims),
`vertices` (V, 3) float32 and `faces` (F, 3) int32, all on the device.  ``save(prefix, space="grid")`` writes
``<prefix>_predicted.obj``, ``<prefix>_voxelized.obj`` (nothing when no voxel is occupied) and ``<prefix>_depthmap.png`` /
``.exr`` as ``SceneNetTrainer.visualize_intermediates`` does (depth columns flipped) and returns the paths.  `space` is the
predicted mesh's: "grid" = lattice index space as ``--test`` writes it; "normalized" = what
``convert_to_scaled_obj.normalize_meshes`` makes of that file (byte for byte); "camera" = metric camera coordinates, the
inverse of ``projection._camera_to_grid(intrinsic, scale_factor)`` (vertices / inf_res first when inf_res > 1: the lattice
index is inf_res times the grid coordinate), in csrc/rgb_preprocess.hip's svr_grid_to_camera.

A ``reconstruct`` result also keeps `image`, the (Hi, Wi, 3) uint8 device tensor the network saw (after the flip, before the
pad), and `pixel_map` (``input_pixel_map``).  ``colorize()`` puts that image back onto the predicted mesh: `colors` (V, 3)
uint8 and `color_state` (V,) uint8 (util/mesh_color.py).  ``save(prefix, color=True)`` also writes
``<prefix>_predicted.ply`` (key "predicted_ply"): the vertices in `space` with those colours; without `color` nothing changes.

``python -m svr_amd.reconstruct --checkpoint C (--rgb a.png [b.png ...] | --distance d.exr) --out DIR [--inf_res n]
[--block s] [--space grid|normalized|camera] [--flip] [--color [--color_bias metres]] [--keep_largest]
[--min_component_faces N] [--min_component_extent CELLS] [--drop_unseen] [--smooth ITERATIONS [--smooth_lambda L]
[--smooth_mu M]] [--simplify CELLS] [--normals] [--preview [K]] [--preview_size H W] [--preview_ssaa S]`` prints one line per
view: the written paths, vertex and face counts and, with ``--color``, ``seen= spread= unreached=``, the vertices per colour
state; with ``--preview``, ``previews=K`` at its end.

``clean(keep_largest=False, min_faces=0, min_extent=0.0, drop_unseen=False)`` drops connected components of the predicted
mesh, the floaters an occupancy network leaves beside the surface (util/mesh_clean.py), and keeps
`components` and `kept`.  Nothing calls it by default.  On the command line the size criteria (``--keep_largest``,
``--min_component_faces``, ``--min_component_extent``) run first; ``--drop_unseen`` (needs ``--color``) then colours the mesh
and drops the components the camera sees no vertex of; ``--color`` finally colours the mesh that is written.  With any of
the four the line ends in ``components=C kept=K``: the components of the raw mesh and how many of them were written.

``simplify(cell=1.0)`` merges the vertices inside each cube of `cell` grid cells per edge into their mean and drops the faces
that collapse or repeat (util/mesh_simplify.py); it keeps `vertex_cluster` and forgets the colours.
Nothing calls it by default.  ``--simplify CELLS`` runs it after the component filters and before ``--color`` colours the
mesh that is written, so ``--drop_unseen`` still decides on the unsimplified mesh; the counts printed are the written mesh's.

``smooth(iterations=10, lam=0.5, mu=-0.53, fix_boundary=True)`` moves the vertices by Taubin's lambda|mu iteration
(util/mesh_smooth.py) and keeps `smooth_state`; faces, components, clusters and colours stay.  Nothing
calls it by default.  ``--smooth ITERATIONS [--smooth_lambda L] [--smooth_mu M]`` runs it after the component flags and before
``--simplify``, so the clusters average smoothed positions.

``normals()`` computes area-weighted vertex normals (util/mesh_render.py) and keeps `vertex_normals` and
`normal_state`; ``render(yaw=0, pitch=0, dolly=0, size=None, ssaa=2, color=None, shading="smooth")`` returns a shaded
(H, W, 3) uint8 picture of the mesh from the input camera, or with the mesh turned in front of it; ``clean()``,
``simplify()`` and ``smooth()`` forget the normals.  ``save(prefix, normals=True)`` writes `vn` lines into
``<prefix>_predicted.obj``; ``save(prefix, preview=k)`` writes ``<prefix>_preview.png`` (the input camera; key "preview") and
``<prefix>_preview_1.png`` ... ``_preview_{k-1}.png`` (yaws spread evenly over +-30 degrees at pitch 10 degrees).  Nothing
calls them by default, and without them every file is byte for byte what it was.  ``--normals`` and ``--preview [K]`` (K = 1
when given without a number; ``--preview_size H W``, ``--preview_ssaa S``) do the same from the command line, on the mesh that
is written, with its colours when ``--color`` is set."""
import argparse
import os
from pathlib import Path

import numpy as np
import torch
from PIL import Image

from . import ops
from .data_processing import sample_io
from .data_processing.distance_to_depth import FromDistanceToDepth, get_intrinsic
from .model.ifnet import implicit_to_vertices
from .util.mesh_color import DEFAULT_FILL, IDENTITY_MAP, vertex_colors
from .util.visualize import export_obj, export_ply, save_png, visualize_depthmap, visualize_grid

SPACES = ("grid", "normalized", "camera")


class Reconstruction:
    """One view's result (module docstring)."""

    def __init__(self, depth, point_cloud, voxel_occupancy, vertices, faces, scale_factor, inf_res, scale_shift, intrinsic=None,
                 image=None, pixel_map=None):
        self.depth, self.point_cloud, self.voxel_occupancy = depth, point_cloud, voxel_occupancy
        self.vertices, self.faces = vertices, faces
        self._scale_factor, self._inf_res, self._scale_shift = scale_factor, int(inf_res), scale_shift
        self._intrinsic = intrinsic                     # 4x4 of the input camera; None: the pipeline's default
        self.image = image                              # (Hi, Wi, 3) uint8 on the device: what the network saw; None: a depth-only result
        self.pixel_map = IDENTITY_MAP if pixel_map is None else tuple(pixel_map)      # depth-map pixel -> image position
        self.colors = self.color_state = None           # colorize()'s results
        self.components = self.kept = None              # clean()'s: the statistics before the filter, the flag per component
        self.vertex_cluster = None                      # simplify()'s: where each vertex of the mesh before it went
        self.smooth_state = None                        # smooth()'s: which vertices it moved
        self.vertex_normals = self.normal_state = None  # normals()'s results

    def _camera_consts(self):
        K = self._intrinsic if self._intrinsic is not None else get_intrinsic()
        return [float(K[0][0]), float(K[0][2]), float(K[1][2])] + [float(v) for v in self._scale_shift] + [0.0, 0.0, 0.0]

    def render_depth(self, size=None, **kw):
        """The predicted mesh ray-cast from the input camera (data_processing.render_view.render_depth; `kw` goes there):
        the (H, W) depth map on the device, 0 where no face is hit, or None when the mesh has no face.  `size` defaults to
        the input depth map's.  The vertices are divided by inf_res first, as vertices_in("camera") does."""
        from .data_processing.render_view import render_depth
        if self.faces is None or int(self.faces.shape[0]) == 0:
            return None
        consts = self._camera_consts()
        if size is None:
            size = tuple(self.depth.shape[-2:]) if self.depth is not None else (240, 320)
        v = self.vertices if self._inf_res == 1 else self.vertices / float(self._inf_res)
        as_host = lambda t: t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)      # noqa: E731
        return render_depth((as_host(v), as_host(self.faces)), size=size, consts=consts, **kw)

    def normals(self):
        """Area-weighted unit normals of the predicted mesh's vertices (util.mesh_render.vertex_normals):
        stores and returns `vertex_normals` (V, 3) float32 and `normal_state` (V,) uint8 (0 has a normal, 1 in no valid face or
        a zero sum, 3 not usable) on the device.  They are those of the mesh as stored, in lattice index space, and follow the
        faces' winding; ``clean()``, ``simplify()`` and ``smooth()`` forget them."""
        from .util.mesh_render import vertex_normals
        self.vertex_normals, self.normal_state = vertex_normals(self.vertices, self.faces)
        return self.vertex_normals, self.normal_state

    def normals_in(self, space):
        """The stored normals (``normals()`` first when there are none) as the unit normals of ``vertices_in(space)``:
        "grid" the stored tensor; "camera" and "normalized" scale the axes (by 1 / s00, 1 / s11, 1 / s22 and by 1 / dims), so
        the normals go through util.mesh_render.transform_normals with that diagonal matrix -> a float32 numpy array."""
        from .util.mesh_render import transform_normals
        if self.vertex_normals is None:
            self.normals()
        if space == "grid":
            return self.vertex_normals
        if space == "normalized":
            scale = np.round(self._scale_factor).astype(np.int64) / np.array([139, 104, 112], dtype=np.float64)
        elif space == "camera":
            scale = 1.0 / np.array([float(self._scale_shift[i]) for i in (0, 2, 4)], dtype=np.float64)
        else:
            raise ValueError(f"space must be one of {SPACES}, got {space!r}")
        return transform_normals(self.vertex_normals.cpu().numpy(), np.diag(np.append(scale, 1.0)))

    def render(self, yaw=0.0, pitch=0.0, dolly=0.0, size=None, ssaa=2, color=None, shading="smooth", **kw):
        """A shaded picture of the predicted mesh (util.mesh_render.render_mesh; `kw` goes there: ambient, albedo, background,
        tile, ...) -> (H, W, 3) uint8 on the device.  yaw = pitch = dolly = 0 is the input camera's view; otherwise the mesh
        is turned in front of that camera by ``orbit_transform`` (`yaw`, `pitch` in degrees, `dolly` in grid cells along the
        optical axis).  `size` defaults to the input depth map's.  `color`: None uses `colors` when they are stored, True
        runs ``colorize()`` first when they are not, False shades the grey `albedo`; a (V, 3) uint8 array is used as given.
        The vertices are divided by inf_res first, as ``render_depth`` does.  A mesh without faces gives an image of
        `background`."""
        from .util.mesh_render import orbit_transform, render_mesh
        if size is None:
            size = tuple(self.depth.shape[-2:]) if self.depth is not None else (240, 320)
        if color is None or color is True:
            if color is True and self.colors is None:
                self.colorize()
            colors = self.colors
        else:
            colors = None if color is False else color
        consts = self._camera_consts()
        v = self.vertices if self._inf_res == 1 else self.vertices / float(self._inf_res)
        transform = None
        if (yaw, pitch, dolly) != (0, 0, 0) and int(self.faces.shape[0]):
            transform = orbit_transform(v, self.faces, yaw, pitch, dolly, consts=consts)
        return render_mesh(v, self.faces, consts=consts, size=size, colors=colors, shading=shading, transform=transform, ssaa=ssaa, **kw)

    def vertices_in(self, space):
        """The predicted mesh's vertices in `space`: a device tensor ("grid", "camera") or a float32 numpy array ("normalized":
        normalize_meshes' float64 formula, rounded once)."""
        if space == "grid":
            return self.vertices
        if space == "normalized":
            dims = np.array([139, 104, 112], dtype=np.float64) / np.round(self._scale_factor).astype(np.int64)
            # normalize_meshes starts from the FILE: the float64 nearest to each vertex's 9-digit decimal, not the widened float32
            v = self.vertices.cpu().numpy()
            v = np.char.mod("%.9g", v.reshape(-1)).astype(np.float64).reshape(v.shape)
            return ((v - dims / 2) / dims).astype(np.float32)
        if space == "camera":
            v = self.vertices if self._inf_res == 1 else self.vertices / float(self._inf_res)
            return ops.grid_to_camera(v, self._scale_shift)
        raise ValueError(f"space must be one of {SPACES}, got {space!r}")

    def colorize(self, image=None, bias=None, spread=True, fill=DEFAULT_FILL, max_passes=None, pixel_map=None):
        """Colour the predicted mesh's vertices from the input image (util.mesh_color.vertex_colors):
        the mesh is ray-cast from the input camera at the depth map's size (``render_depth``), a vertex that render sees takes
        the image's bilinear sample at its projection, and with `spread` the others take colour along mesh edges.  Stores and
        returns `colors` (V, 3) uint8 and `color_state` (V,) uint8 (1 seen, 2 spread, 0 unreached = `fill`) on the device.
        `image` (anything ``reconstruct`` takes) replaces the stored image and then maps through `pixel_map` (ax, bx, ay, by;
        default the identity); a ``reconstruct_depth`` result stores no image and needs it.  `bias`: vertex_colors' (None: one
        grid cell)."""
        if image is not None:
            img = _pixels(image)
            img = (img if torch.is_tensor(img) else torch.from_numpy(img)).to(self.vertices.device).contiguous()
            pm = IDENTITY_MAP if pixel_map is None else tuple(pixel_map)
        elif self.image is not None:
            img, pm = self.image, self.pixel_map if pixel_map is None else tuple(pixel_map)
        else:
            raise RuntimeError("colorize: this result was reconstructed from a depth map and holds no image to take colours "
                               "from; pass image= (and pixel_map= unless its pixels are the depth map's)")
        V = int(self.vertices.shape[0])
        depth = self.render_depth()
        if depth is None:                                # no face: nothing is seen, nothing spreads
            self.colors = torch.tensor(fill, dtype=torch.uint8, device=self.vertices.device).repeat(V, 1)
            self.color_state = torch.zeros(V, dtype=torch.uint8, device=self.vertices.device)
            return self.colors, self.color_state
        v = self.vertices if self._inf_res == 1 else self.vertices / float(self._inf_res)
        self.colors, self.color_state = vertex_colors(v, self.faces, img, depth, self._camera_consts(), pixel_map=pm, bias=bias,
                                                      spread=spread, fill=fill, max_passes=max_passes)
        return self.colors, self.color_state

    def clean(self, keep_largest=False, min_faces=0, min_extent=0.0, drop_unseen=False):
        """Drop connected components of the predicted mesh (util.mesh_clean): the closed blobs an
        occupancy network leaves in free space.  A component stays iff it has at least max(1, `min_faces`) faces, its bounding
        box's diagonal is at least `min_extent` grid cells (multiplied by inf_res here: the vertices are lattice indices) and,
        with `drop_unseen`, the camera sees at least one of its vertices (``color_state == 1``; runs ``colorize()`` first when
        no state is stored, so a depth-only result without colours raises "holds no image"); with `keep_largest` only the one
        with the most faces among those.  Replaces `vertices` and `faces`, stores `components` (the statistics BEFORE the
        filter) and `kept` (the flag per component), and returns self; keeping nothing leaves an empty mesh.
        `colors` and `color_state`, when stored, are carried along by index: they stay those of the UNFILTERED mesh's render,
        in which a dropped component may have hidden what is now visible; a second ``colorize()`` recomputes them."""
        from .util.mesh_clean import clean_mesh
        mark = None
        if drop_unseen:
            if self.color_state is None:
                self.colorize()
            mark = (self.color_state == 1).to(torch.uint8)
        vertices, faces, index, self.components, self.kept = clean_mesh(
            self.vertices, self.faces, mark, keep_largest=keep_largest, min_faces=min_faces,
            min_extent=float(min_extent) * self._inf_res, require_mark=bool(drop_unseen))
        self.vertices, self.faces = vertices, faces
        self.vertex_normals = self.normal_state = None
        if self.colors is not None:
            self.colors, self.color_state = self.colors[index.long()], self.color_state[index.long()]
        return self

    def simplify(self, cell=1.0):
        """Simplify the predicted mesh by vertex clustering (util.mesh_simplify): the vertices inside
        one cube of `cell` grid cells per edge (multiplied by inf_res here: the vertices are lattice indices) become one vertex
        at their mean, and the faces that collapse or repeat are dropped.  Replaces `vertices` and `faces`, stores
        `vertex_cluster` (per vertex of the mesh BEFORE the call, its new vertex or -1) and returns self.  `colors` and
        `color_state` are reset to None: a cluster's vertex is a new position, so ``save(color=True)`` (or ``colorize()``)
        colours the simplified mesh from the image there instead of pooling the old colours.  `components` and `kept` stay:
        they describe the raw mesh.  A mesh without faces is returned unchanged."""
        from .util.mesh_simplify import simplify_mesh
        if self.faces is None or int(self.faces.shape[0]) == 0:
            return self
        out = simplify_mesh(self.vertices, self.faces, float(cell) * self._inf_res)
        self.vertices, self.faces, self.vertex_cluster = out.vertices, out.faces, out.vertex_cluster
        self.colors = self.color_state = None
        self.vertex_normals = self.normal_state = None
        return self

    def smooth(self, iterations=10, lam=0.5, mu=-0.53, fix_boundary=True):
        """Smooth the predicted mesh with Taubin's lambda|mu iteration (util.mesh_smooth): takes the
        terraces out of the marching-cubes surface of a near-binary field without shrinking it.  With `fix_boundary` the rims
        the lattice border cut open stay on the border.  Replaces `vertices`, stores `smooth_state` (per vertex: 0 moved, 1 in
        no face, 2 held on a boundary, 3 not usable) and returns self.  `faces`, `components`, `kept`, `vertex_cluster`,
        `colors` and `color_state` stay: the indices are unchanged and a position moves by less than a cell or so, so the
        colours are still those of the image at (nearly) that place; a second ``colorize()`` resamples them at the smoothed
        positions.  `smooth_state`, like `vertex_cluster`, describes the mesh the call saw: a later ``clean()`` or ``simplify()``
        renumbers the vertices and leaves it as it is.  A mesh without faces is returned unchanged."""
        from .util.mesh_smooth import smooth_mesh
        if self.faces is None or int(self.faces.shape[0]) == 0:
            return self
        out = smooth_mesh(self.vertices, self.faces, iterations=iterations, lam=lam, mu=mu, fix_boundary=fix_boundary)
        self.vertices, self.smooth_state = out.vertices, out.state
        self.vertex_normals = self.normal_state = None
        return self

    def save(self, prefix, space="grid", color=False, normals=False, preview=0, preview_size=None, preview_ssaa=2):
        """Module docstring; `normals` writes `vn` lines into ``_predicted.obj`` (``normals_in(space)``); `preview` = k > 0 writes
        k pictures of the mesh (``render``, at `preview_size`, default the depth map's, and `preview_ssaa`):
        ``<prefix>_preview.png`` from the input camera (key "preview") and ``<prefix>_preview_1.png`` ...
        ``_preview_{k-1}.png`` (keys "preview_1" ...) at pitch 10 degrees and the k - 1 yaws of
        ``numpy.linspace(-30, 30, k - 1)``.  The defaults write what was always written."""
        if isinstance(preview, bool) or int(preview) != preview or preview < 0:
            raise ValueError(f"save: preview={preview!r} (need a number of pictures, 0 for none)")
        vertices = self.vertices_in(space)
        prefix = os.fspath(prefix)
        if os.path.dirname(prefix):
            os.makedirs(os.path.dirname(prefix), exist_ok=True)
        paths = {"predicted": prefix + "_predicted.obj", "voxelized": prefix + "_voxelized.obj",
                 "depthmap_png": prefix + "_depthmap.png", "depthmap_exr": prefix + "_depthmap.exr"}
        vox = self.voxel_occupancy
        visualize_grid(vox.reshape(vox.shape[-3:]), paths["voxelized"])
        export_obj(vertices, self.faces, paths["predicted"], normals=self.normals_in(space) if normals else None)
        visualize_depthmap(self.depth, prefix + "_depthmap", flip=True)
        if not os.path.exists(paths["voxelized"]):
            del paths["voxelized"]
        if color:
            if self.colors is None:
                self.colorize()
            paths["predicted_ply"] = prefix + "_predicted.ply"
            export_ply(vertices, self.faces, self.colors, paths["predicted_ply"])
        for i in range(int(preview)):
            key = "preview" if i == 0 else f"preview_{i}"
            paths[key] = prefix + "_" + key + ".png"
            view = {} if i == 0 else {"yaw": float(np.linspace(-30.0, 30.0, int(preview) - 1)[i - 1]), "pitch": 10.0}
            save_png(self.render(size=preview_size, ssaa=preview_ssaa, **view), paths[key])
        return paths


def input_pixel_map(Hi, Wi, resize_input):
    """(ax, bx, ay, by): where depth-map pixel (u, v) of the 240 x 320 output lies in the (Hi, Wi) image the network saw.
    Without resize_input the two grids coincide.  With it, ops.rgb_preprocess pads the image to a square (pad = (m - n) // 2 on
    both sides of the shorter axis), the network works on the resized square, and the depth map is rows 40..279 of the
    320 x 320 square: pixel centres map linearly, centre (v + 40 + 0.5) / 320 of the square to the same share of the padded
    image.  Positions in the padded border come out outside [-0.5, n - 0.5]."""
    if not resize_input:
        return IDENTITY_MAP
    m = max(Hi, Wi)
    pad_y, pad_x = (m - Hi) // 2, (m - Wi) // 2
    ay, ax = (Hi + 2 * pad_y) / 320, (Wi + 2 * pad_x) / 320
    return (ax, 0.5 * ax - 0.5 - pad_x, ay, 40.5 * ay - 0.5 - pad_y)


def _pixels(image):
    """One input of reconstruct() -> (H, W, 3) uint8, a numpy array or a device tensor."""
    if isinstance(image, (str, os.PathLike)):
        with Image.open(image) as im:
            return np.array(im.convert("RGB"), dtype=np.uint8)
    if isinstance(image, Image.Image):
        return np.array(image.convert("RGB"), dtype=np.uint8)
    a = image if torch.is_tensor(image) else np.asarray(image)
    if a.dtype != (torch.uint8 if torch.is_tensor(a) else np.uint8) or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"reconstruct: an image array must be (H, W, 3) uint8, got {tuple(a.shape)} {a.dtype}")
    return a


class Reconstructor:
    def __init__(self, model, block=None):
        self.model = model.cuda().eval()
        self.block = block

    @classmethod
    def from_checkpoint(cls, path, inf_res=None, scale_factor=None, skip_unet=None, block=None):
        from .trainer.checkpoint import load_checkpoint
        from .trainer.trainer_scene_net import SceneNetTrainer
        ck = load_checkpoint(path)
        hparams = argparse.Namespace(**ck["hyper_parameters"])
        for name, value in (("inf_res", inf_res), ("scale_factor", scale_factor), ("skip_unet", skip_unet)):
            if value is not None:
                setattr(hparams, name, value)
        model = SceneNetTrainer(hparams)
        model.load_state_dict({k: v for k, v in ck["state_dict"].items() if model.unet is not None or not k.startswith("unet.")})
        return cls(model, block)

    @property
    def device(self):
        return next(self.model.ifnet.parameters()).device

    def _views(self, depth, point_cloud, voxel_occupancy, images=None):
        m, h = self.model, self.model.hparams
        dims = m.dims.cpu().numpy().astype(np.int32)
        inf_res = int(getattr(h, "inf_res", 1))
        scale_shift = m.project._consts(h.scale_factor)[3:9]
        views = []
        for i in range(depth.shape[0]):
            vox = voxel_occupancy[i]
            vertices, faces = implicit_to_vertices(m.ifnet, vox.reshape(1, 1, *vox.shape[-3:]), dims, 0.5, inf_res, self.block)
            image = None if images is None else images[i]
            pixel_map = None if images is None else input_pixel_map(int(image.shape[0]), int(image.shape[1]), bool(h.resize_input))
            views.append(Reconstruction(depth[i], point_cloud[i], vox, vertices, faces, h.scale_factor, inf_res, scale_shift,
                                        m.project.intrinsic, image, pixel_map))
        return views

    def preprocess(self, pixels, flip=False):
        """(B, H, W, 3) uint8 device tensor -> the UNet's input, as the dataset's transform makes it."""
        h = self.model.hparams
        return ops.rgb_preprocess(pixels, int(getattr(h, "W", 256)), bool(h.resize_input), flip)

    def reconstruct(self, images, flip=False):
        if self.model.unet is None:
            raise RuntimeError("reconstruct: this model was built with skip_unet and has no UNet to predict a depth map from an "
                               "image; give it a depth map or a distance .exr through reconstruct_depth()")
        single = not isinstance(images, (list, tuple))
        pixels = [_pixels(im) for im in ([images] if single else images)]
        if not self.model.hparams.resize_input and any(tuple(p.shape[:2]) != (240, 320) for p in pixels):
            raise ValueError("reconstruct: a model trained without resize_input takes 240 x 320 images only")
        groups = {}
        for i, p in enumerate(pixels):
            groups.setdefault(tuple(p.shape), []).append(i)
        out = [None] * len(pixels)
        with torch.no_grad():
            for indices in groups.values():
                batch = torch.stack([torch.as_tensor(pixels[i]).to(self.device) for i in indices])
                depth = self.model._predict_depth(self.preprocess(batch, flip))
                seen = batch.flip(2) if flip else batch                # what the network saw, before the pad
                for i, view in zip(indices, self._views(depth, *self.model._voxels_from_depth(depth), images=seen)):
                    out[i] = view
        return out[0] if single else out

    def reconstruct_depth(self, depth):
        h = self.model.hparams
        if isinstance(depth, (str, os.PathLike)):
            distance = sample_io.exr_read(depth, "R")
            depth = FromDistanceToDepth(get_intrinsic(getattr(h, "intrinsics_path", None))[0][0])(distance)
        elif not torch.is_tensor(depth):
            depth = torch.from_numpy(np.ascontiguousarray(depth, dtype=np.float32)).to(self.device)
        elif not depth.is_cuda:
            raise RuntimeError("reconstruct_depth HIP path needs GPU tensors (no CPU fallback)")
        single = depth.dim() == 2
        depth = (depth.unsqueeze(0) if single else depth).float().contiguous()
        if depth.dim() != 3 or tuple(depth.shape[1:]) != (240, 320):
            raise ValueError(f"reconstruct_depth: expected (B, 240, 320) or (240, 320), got {tuple(depth.shape)}")
        with torch.no_grad():
            views = self._views(depth, *self.model._voxels_from_depth(depth))
        return views[0] if single else views


def main(argv=None):
    parser = argparse.ArgumentParser(description="Reconstruct meshes from images with a trained scene network")
    parser.add_argument("--checkpoint", required=True, help="a train_scene_net checkpoint")
    source = parser.add_mutually_exclusive_group(required=True)
    source.add_argument("--rgb", nargs="+", help="image files")
    source.add_argument("--distance", help="a distance .exr (channel R): skips the UNet")
    parser.add_argument("--out", required=True, help="output directory")
    parser.add_argument("--inf_res", type=int, default=None, help="inference lattice per grid cell (default: the checkpoint's)")
    parser.add_argument("--block", type=int, default=None, help="sparse lattice block edge, 0 = dense (default: SVR_INF_BLOCK)")
    parser.add_argument("--space", choices=SPACES, default="grid", help="space of the predicted mesh")
    parser.add_argument("--flip", action="store_true", help="mirror the images left-right first")
    parser.add_argument("--color", action="store_true", help="also write <name>_predicted.ply with vertex colours from the image")
    parser.add_argument("--color_bias", type=float, default=None, help="visibility bias in metres (default: one grid cell)")
    parser.add_argument("--keep_largest", action="store_true", help="keep only the connected component with the most faces")
    parser.add_argument("--min_component_faces", type=int, default=None, metavar="N", help="drop components with fewer than N faces")
    parser.add_argument("--min_component_extent", type=float, default=None, metavar="CELLS",
                        help="drop components whose bounding-box diagonal is shorter than CELLS grid cells")
    parser.add_argument("--drop_unseen", action="store_true", help="drop components the camera sees no vertex of (needs --color)")
    parser.add_argument("--simplify", type=float, default=None, metavar="CELLS",
                        help="merge the vertices inside each cube of CELLS grid cells per edge (vertex clustering; default: off)")
    parser.add_argument("--smooth", type=int, default=None, metavar="ITERATIONS",
                        help="Taubin lambda|mu smoothing of the mesh, ITERATIONS times, rims on the lattice border held (default: off)")
    parser.add_argument("--smooth_lambda", type=float, default=0.5, help="the shrinking step of --smooth, 0 < L <= 1")
    parser.add_argument("--smooth_mu", type=float, default=-0.53, help="the inflating step of --smooth, -1 <= M <= 0 (0: plain Laplacian)")
    parser.add_argument("--normals", action="store_true", help="write vertex normals (vn lines) into <name>_predicted.obj")
    parser.add_argument("--preview", type=int, nargs="?", const=1, default=None, metavar="K",
                        help="write K shaded pictures of the mesh: <name>_preview.png from the input camera, the others from beside it "
                             "(default when given: 1)")
    parser.add_argument("--preview_size", type=int, nargs=2, default=None, metavar=("H", "W"), help="size of the pictures (default: the depth map's)")
    parser.add_argument("--preview_ssaa", type=int, default=2, metavar="S", help="sub-pixels per pixel and axis of the pictures, 1 to 4")
    args = parser.parse_args(argv)
    if args.preview is not None and not args.preview > 0:
        parser.error("--preview needs a positive number of pictures")
    if args.preview_ssaa not in (1, 2, 3, 4):
        parser.error("--preview_ssaa needs 1, 2, 3 or 4")
    if args.smooth is not None and not 0 < args.smooth <= 1024:
        parser.error("--smooth needs a positive number of iterations, 1024 at the most")
    if args.color and args.distance:
        parser.error("--color needs --rgb: a distance map carries no colours")
    if args.drop_unseen and not args.color:
        parser.error("--drop_unseen needs --color: what the camera sees is decided while colouring")
    if args.simplify is not None and not args.simplify > 0:
        parser.error("--simplify needs a positive number of grid cells")
    by_size = args.keep_largest or args.min_component_faces is not None or args.min_component_extent is not None
    cleaning = by_size or args.drop_unseen
    rec =Reconstructor.from_checkpoint(args.checkpoint, inf_res=args.inf_res, skip_unet=True if args.distance else None,
                                        block=args.block)
    if args.distance:
        names, views = [Path(args.distance).stem], [rec.reconstruct_depth(args.distance)]
    else:
        names, views = [Path(p).stem for p in args.rgb], rec.reconstruct(list(args.rgb), flip=args.flip)
    for name, view in zip(names, views):
        counts = parts = ""
        if cleaning:
            total = None                                  # the components of the raw mesh
            if by_size:                                   # the size criteria first ...
                view.clean(keep_largest=args.keep_largest, min_faces=args.min_component_faces or 0,
                           min_extent=args.min_component_extent or 0.0)
                total = view.components.count
            if args.drop_unseen:                          # ... then what the camera sees of the rest
                view.colorize(bias=args.color_bias)
                view.clean(drop_unseen=True)
                total = view.components.count if total is None else total
            parts = f" components={total} kept={int(view.kept.sum())}"
        if args.smooth is not None:                       # after the filters: floaters are dropped, not smoothed
            view.smooth(args.smooth, lam=args.smooth_lambda, mu=args.smooth_mu)
        if args.simplify is not None:                     # after the filters, which saw the raw mesh and its colour states
            view.simplify(args.simplify)
        if args.color:                                    # on the mesh that is written
            _, state = view.colorize(bias=args.color_bias)
            n = torch.bincount(state.long(), minlength=3).tolist()
            counts = f" seen={n[1]} spread={n[2]} unreached={n[0]}"
        paths = view.save(Path(args.out) / name, space=args.space, color=args.color, normals=args.normals, preview=args.preview or 0,
                          preview_size=args.preview_size, preview_ssaa=args.preview_ssaa)
        shown = "" if args.preview is None else f" previews={args.preview}"
        print(" ".join(paths.values()), f"vertices={view.vertices.shape[0]} faces={view.faces.shape[0]}" + counts + parts + shown)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
