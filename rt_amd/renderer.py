"""``HipRayTracer`` — the harness-side handle on one ``rt_hip_ctx`` (one GPU).

Mirrors the lifetime and the call shape of a renderer in the reference: created once
(``renderers::description::create``, reference src/renderer.hpp:39), asked to ``render(scene, pixels)``
(src/renderer.hpp:11, src/renderers/mg_ray_tracer.cpp:178), destroyed through ``close()``.

Two ways in, both straight through the C ABI of include/rt_hip.h:

* ``render(scene_pod, width, height, ...)`` -> numpy ``uint32[H, W]`` : the drop-in ``rt_hip_render`` (upload,
  kernels, copy into a HOST frame) — what the reference-side shim calls.
* ``upload`` + ``render_device`` (+ ``assemble_device``): the scene stays resident in HBM and frames are
  written to DEVICE buffers (raw pointers, e.g. of torch tensors) on a caller-chosen stream — what
  ``bench.py`` and the multi-GPU path use.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .capi import RtHipAdaptiveInfo, RtHipAdaptiveParams, RtHipBloomInfo, RtHipBloomParams, RtHipDenoiseParams, RtHipPartition, RtHipPhases, RtHipProgress, RtHipScene, RtHipStats, RtHipTemporalInfo, RtHipTemporalParams, RtHipTonemapInfo, RtHipTonemapParams, RtHipUpsampleParams, RtHipUpscaleInfo, check


def local_rows(height: int, rank: int, world: int, stripe_rows: int = capi.RT_HIP_DEFAULT_STRIPE_ROWS) -> int:
    out = C.c_uint32()
    check(capi.hip_lib().rt_hip_local_rows(height, C.byref(RtHipPartition(rank, world, stripe_rows)), C.byref(out)))
    return out.value


def padded_local_rows(height: int, world: int, stripe_rows: int = capi.RT_HIP_DEFAULT_STRIPE_ROWS) -> int:
    out = C.c_uint32()
    check(capi.hip_lib().rt_hip_padded_local_rows(height, C.byref(RtHipPartition(0, world, stripe_rows)), C.byref(out)))
    return out.value


def scene_check(scene: RtHipScene) -> int:
    """rt_hip_scene_check: validate the columns as rt_hip_render would and return their fingerprint (pure host code)."""
    out = C.c_uint64()
    check(capi.hip_lib().rt_hip_scene_check(C.byref(scene), C.byref(out)))
    return out.value


def unique_id() -> bytes:
    """A fresh id for a renderer with one process per GPU (rt_hip_unique_id): create it once, give it to every rank."""
    buf = (C.c_char * 128)()
    check(capi.hip_lib().rt_hip_unique_id(buf))
    return bytes(buf.raw)


def live_frame_locks() -> int:
    """rt_hip_live_frame_locks: page-locks on callers' memory that contexts of this process hold right now."""
    return int(capi.hip_lib().rt_hip_live_frame_locks())


def bvh_build(scene: RtHipScene) -> dict:
    """The sphere hierarchy RT_HIP_FLAG_BVH builds for `scene`, built on the host (rt_hip_kat_bvh_build; no GPU needed):
    nodes float32[N, 16] (links as bits in words 3 and 7), order / always uint32, spheres float32[T, 4] (leaf order),
    bound float32[4] (centre, radius), depth, root."""
    n = max(int(scene.n_spheres), 1)
    counts = np.zeros(5, dtype=np.uint32)
    nodes = np.zeros((n, 16), dtype=np.float32)
    order = np.zeros(n, dtype=np.uint32)
    spheres = np.zeros((n, 4), dtype=np.float32)
    always = np.zeros(n, dtype=np.uint32)
    bound = np.zeros(4, dtype=np.float32)
    capi.check_kat(capi.kat_lib().rt_hip_kat_bvh_build(C.byref(scene), counts.ctypes.data, nodes.ctypes.data, order.ctypes.data, spheres.ctypes.data, always.ctypes.data, bound.ctypes.data))
    n_nodes, n_tree, n_always, depth, root = (int(c) for c in counts)
    return {"nodes": nodes[:n_nodes], "order": order[:n_tree], "spheres": spheres[:n_tree], "always": always[:n_always], "bound": bound, "depth": depth, "root": root}


def box_bvh_build(scene: RtHipScene) -> dict:
    """The box hierarchy RT_HIP_FLAG_BOX_BVH builds for `scene`, built on the host (rt_hip_kat_box_bvh_build; no GPU needed):
    nodes float32[N, 16] (links as bits in words 3 and 7), order / always uint32, corners float32[T, 8] (leaf order), depth, root."""
    n = max(int(scene.n_boxes), 1)
    counts = np.zeros(5, dtype=np.uint32)
    nodes = np.zeros((n, 16), dtype=np.float32)
    order = np.zeros(n, dtype=np.uint32)
    corners = np.zeros((n, 8), dtype=np.float32)
    always = np.zeros(n, dtype=np.uint32)
    capi.check_kat(capi.kat_lib().rt_hip_kat_box_bvh_build(C.byref(scene), counts.ctypes.data, nodes.ctypes.data, order.ctypes.data, corners.ctypes.data, always.ctypes.data))
    n_nodes, n_tree, n_always, depth, root = (int(c) for c in counts)
    return {"nodes": nodes[:n_nodes], "order": order[:n_tree], "corners": corners[:n_tree], "always": always[:n_always], "depth": depth, "root": root}


def upsample_default_params() -> RtHipUpsampleParams:
    """rt_hip_upsample_default_params: what a NULL `params` stands for (pure host code)."""
    params = RtHipUpsampleParams()
    check(capi.hip_lib().rt_hip_upsample_default_params(C.byref(params)))
    return params


def upsample_low_size(width: int, height: int, factor: int) -> tuple:
    """rt_hip_upsample_low_size: the (width, height) of the frame render_upscaled traces for `factor` (pure host code)."""
    w, h = C.c_uint32(0), C.c_uint32(0)
    check(capi.hip_lib().rt_hip_upsample_low_size(width, height, factor, C.byref(w), C.byref(h)))
    return w.value, h.value


def tonemap_default_params() -> RtHipTonemapParams:
    """rt_hip_tonemap_default_params: what a NULL `params` of the tone-mapping entry points stands for (pure host code)."""
    params = RtHipTonemapParams()
    check(capi.hip_lib().rt_hip_tonemap_default_params(C.byref(params)))
    return params


def bloom_default_params() -> RtHipBloomParams:
    """rt_hip_bloom_default_params: what a NULL `params` of the bloom entry points stands for (pure host code)."""
    params = RtHipBloomParams()
    check(capi.hip_lib().rt_hip_bloom_default_params(C.byref(params)))
    return params


def bloom_from_spec(spec: str) -> RtHipBloomParams:
    """rt_hip_bloom_from_spec: ``default``, or the defaults with the ``KEY=VALUE`` items of the text (intensity, threshold, knee, scatter,
    levels; separated by ','; pure host code).  Raises RtHipError with the text in the message for anything else."""
    params = RtHipBloomParams()
    check(capi.hip_lib().rt_hip_bloom_from_spec(spec.encode(), C.byref(params)))
    return params


def bloom_plan(width: int, height: int, params: RtHipBloomParams | None = None) -> dict:
    """rt_hip_bloom_plan: the pyramid a width x height frame gets — levels, last_width, last_height, scratch_bytes (pure host code)."""
    info = RtHipBloomInfo()
    check(capi.hip_lib().rt_hip_bloom_plan(width, height, C.byref(params) if params is not None else None, C.byref(info)))
    return info.as_dict()


def tonemap_from_spec(spec: str) -> RtHipTonemapParams:
    """rt_hip_tonemap_from_spec: the defaults with the curve and the exposure of ``CURVE[:EXPOSURE]`` (none, reinhard or aces; auto or
    a positive number; pure host code).  Raises RtHipError with the text in the message for anything else."""
    params = RtHipTonemapParams()
    check(capi.hip_lib().rt_hip_tonemap_from_spec(spec.encode(), C.byref(params)))
    return params


def denoise_default_params() -> RtHipDenoiseParams:
    """rt_hip_denoise_default_params: what a NULL `params` stands for (pure host code)."""
    params = RtHipDenoiseParams()
    check(capi.hip_lib().rt_hip_denoise_default_params(C.byref(params)))
    return params


def temporal_default_params() -> RtHipTemporalParams:
    """rt_hip_temporal_default_params: what a NULL `temporal` stands for (pure host code)."""
    params = RtHipTemporalParams()
    check(capi.hip_lib().rt_hip_temporal_default_params(C.byref(params)))
    return params


def adaptive_default_params() -> RtHipAdaptiveParams:
    """rt_hip_adaptive_default_params: what a NULL `params` of the adaptive entry points stands for (pure host code)."""
    params = RtHipAdaptiveParams()
    check(capi.hip_lib().rt_hip_adaptive_default_params(C.byref(params)))
    return params


def lens_from_spec(spec: str) -> capi.RtHipLens:
    """rt_hip_lens_from_spec: a lens from ``aperture=A,focus=F`` (pure host code).  Raises RtHipError for a malformed spec."""
    lens = capi.RtHipLens()
    check(capi.hip_lib().rt_hip_lens_from_spec(spec.encode(), C.byref(lens)))
    return lens


def lights_from_spec(spec: str, material_names=None, n_materials: int | None = None) -> np.ndarray:
    """rt_hip_lights_from_spec: an emission table float32[n_materials, 3] from ``KEY=R,G,B;KEY=V;...`` (pure host code).  An
    all-digit KEY is a material index, any other a material name (every material of that name).  Raises RtHipError with the item
    in the message for a malformed spec."""
    names = list(material_names) if material_names is not None else None
    n = len(names) if n_materials is None else n_materials
    table = np.zeros((n, 3), dtype=np.float32)
    c_names = (C.c_char_p * max(n, 1))(*[name.encode() for name in names]) if names is not None else None
    check(capi.hip_lib().rt_hip_lights_from_spec(spec.encode(), c_names, n, table.ctypes.data_as(capi.c_float_p)))
    return table


def device_count() -> int:
    n = C.c_int()
    check(capi.hip_lib().rt_hip_device_count(C.byref(n)))
    return n.value


class HipRayTracer:
    """`device`: one GPU (rt_hip_create).  `devices`: a list of GPUs behind ONE render() call (rt_hip_create_multi):
    scene replicated, row stripes dealt round-robin, one RCCL gather to devices[0], one copy to the host.
    `peer_copy`: move the stripes with hipMemcpyPeerAsync instead of RCCL (allows a device to appear twice: tests).
    `direct_frame`: no gather — every member stores its pixels straight into the caller's page-locked back buffer."""

    _progressive_size = (1, 1)  # (width, height) render_progressive was last asked for

    def __init__(self, device: int = 0, devices: list[int] | None = None, peer_copy: bool = False, direct_frame: bool = False, rank: int | None = None, world: int | None = None, unique_id: bytes | None = None):
        """`rank`, `world`, `unique_id`: one rank of a renderer with one process per GPU (rt_hip_create_rank; collective).
        The id comes from `unique_id()` on one process and must reach every rank unchanged."""
        self._lib = capi.hip_lib()
        self._ctx = C.c_void_p()
        if rank is not None:
            assert world is not None and unique_id is not None and len(unique_id) == 128
            check(self._lib.rt_hip_create_rank(C.byref(self._ctx), device, rank, world, (C.c_char * 128).from_buffer_copy(unique_id)))
            self.device = device
            self.devices = [device]
            self.rank, self.world = rank, world
            return
        self.rank, self.world = 0, 1
        if devices is None:
            check(self._lib.rt_hip_create(C.byref(self._ctx), device))
            self.device = device
            self.devices = [device]
        else:
            ordinals = (C.c_int * len(devices))(*devices)
            check(self._lib.rt_hip_create_multi(C.byref(self._ctx), ordinals, len(devices), (capi.RT_HIP_MULTI_PEER_COPY if peer_copy else 0) | (capi.RT_HIP_MULTI_DIRECT_FRAME if direct_frame else 0)))
            self.device = devices[0]
            self.devices = list(devices)

    def join_ranks(self, rank: int, world: int, unique_id: bytes, timeout_ms: int = 0) -> None:
        """rt_hip_join_ranks: the collective half of rt_hip_create_rank, on a context made by plain ``HipRayTracer(device)``
        — after the launcher has made sure that EVERY rank holds one.  Raises RtHipError (RT_HIP_TIMEOUT after `timeout_ms`;
        the tracer stays a usable single-GPU tracer then)."""
        assert len(unique_id) == 128
        check(self._lib.rt_hip_join_ranks(self._ctx, rank, world, (C.c_char * 128).from_buffer_copy(unique_id), timeout_ms))
        self.rank, self.world = rank, world

    def join_frame_group(self, rank: int, world: int, name: str, timeout_ms: int = 0) -> None:
        """rt_hip_join_frame_group: one process per GPU without an exchange step.  On a context made by plain
        ``HipRayTracer(device)``, collectively; afterwards EVERY rank calls ``render(..., out=<its mapping of the one shared
        uint32[H, W] buffer>)`` and every call returns when the whole frame is in that buffer.  `name`: a fresh shm_open name
        ("/rt_hip_...") all ranks were handed.  Raises RtHipError (RT_HIP_TIMEOUT after `timeout_ms`)."""
        check(self._lib.rt_hip_join_frame_group(self._ctx, rank, world, name.encode(), timeout_ms))
        self.rank, self.world, self.shared_frame = rank, world, True

    def comm_info(self, member: int = 0) -> dict:
        """What RCCL reports about the communicator member `member` talks through (rt_hip_comm_info)."""
        ranks, rank, device, transport = C.c_int(), C.c_int(), C.c_int(), C.c_uint32()
        check(self._lib.rt_hip_comm_info(self._ctx, member, C.byref(ranks), C.byref(rank), C.byref(device), C.byref(transport)))
        return {"ranks": ranks.value, "rank": rank.value, "device": device.value, "transport": capi.TRANSPORT_NAMES.get(transport.value, str(transport.value))}

    def phases(self) -> dict:
        """Where the time of the most recent render() went (rt_hip_phases_fetch)."""
        phases = RtHipPhases()
        check(self._lib.rt_hip_phases_fetch(self._ctx, C.byref(phases)))
        return phases.as_dict()

    def close(self) -> None:
        ctx, self._ctx = getattr(self, "_ctx", None), None
        if ctx:
            self._lib.rt_hip_destroy(ctx)

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_emission(self, emission=None) -> None:
        """rt_hip_set_emission: the context's emission table, float32[n_materials, 3] (None clears it).  A material whose row has a
        component above 0 is a light in frames rendered with RT_HIP_FLAG_EMISSION; the table is copied, survives
        scene uploads and reaches every member device."""
        if emission is None:
            check(self._lib.rt_hip_set_emission(self._ctx, None, 0))
            return
        table = np.ascontiguousarray(emission, dtype=np.float32).reshape(-1, 3)
        check(self._lib.rt_hip_set_emission(self._ctx, table.ctypes.data_as(capi.c_float_p), len(table)))

    def set_lens(self, aperture_radius: float | None = None, focus_distance: float = 1.0) -> None:
        """rt_hip_set_lens: the context's thin lens (None clears it).  Frames rendered with RT_HIP_FLAG_THIN_LENS start their primary
        rays on a disk of that radius around the eye and are sharp on the plane `focus_distance` along the view direction
        (DESIGN.md §3.17); the lens is copied, survives scene uploads and reaches every member device."""
        if aperture_radius is None:
            check(self._lib.rt_hip_set_lens(self._ctx, None))
            return
        check(self._lib.rt_hip_set_lens(self._ctx, C.byref(capi.RtHipLens(aperture_radius, focus_distance))))

    # ---- drop-in ------------------------------------------------------------------------------------------
    def render(self, scene: RtHipScene, width: int, height: int, seed: int = 1, flags: int = 0, want_rgb: bool = False, out: np.ndarray | None = None, stats: bool = True):
        """rt_hip_render: returns (rgba8 uint32[H, W], rgb float32[H, W, 3] or None, stats dict).

        `out`: a uint32[H, W] array to render into (like rt's persistent back buffer); a fresh one otherwise.
        `stats=False`: the call as the plug-in makes it (stats == NULL): nothing but the launch and the wait is enqueued;
        the returned dict is empty."""
        want_stats = stats
        stats = RtHipStats()
        stats_arg = C.byref(stats) if want_stats else None
        if self.rank != 0 and not getattr(self, "shared_frame", False):  # a rank whose rank 0 lives in another process renders and sends; it has no frame of its own
            rgb = np.empty((height, width, 3), dtype=np.float32) if want_rgb else None
            check(self._lib.rt_hip_render(self._ctx, C.byref(scene), None, width, height, seed, flags, rgb.ctypes.data if rgb is not None else None, stats_arg))
            return None, None, stats.as_dict() if want_stats else {}
        rgba = out if out is not None else np.empty((height, width), dtype=np.uint32)
        assert rgba.dtype == np.uint32 and rgba.shape == (height, width) and rgba.flags.c_contiguous
        rgb = np.empty((height, width, 3), dtype=np.float32) if want_rgb else None
        check(
            self._lib.rt_hip_render(
                self._ctx,
                C.byref(scene),
                rgba.ctypes.data,
                width,
                height,
                seed,
                flags,
                rgb.ctypes.data if rgb is not None else None,
                stats_arg,
            )
        )
        return rgba, rgb, stats.as_dict() if want_stats else {}

    def render_progressive(self, scene: RtHipScene, width: int, height: int, seed: int = 1, flags: int = 0, pass_samples: int = 16, want_rgb: bool = False, out: np.ndarray | None = None, stats: bool = True):
        """rt_hip_render_progressive: the next `pass_samples` samples per pixel (0 = all that is left) of the frame in flight —
        or of a new one, if anything the frame depends on changed.  Returns (rgba8 uint32[H, W], rgb float32[H, W, 3] or None,
        stats dict of THIS pass, progress dict: samples_done, samples_total, passes, restarted).  The frame returned is the
        one-shot frame at samples_per_pixel = samples_done, bit for bit."""
        stats_pod, progress = RtHipStats(), RtHipProgress()
        rgba = out if out is not None else np.empty((height, width), dtype=np.uint32)
        assert rgba.dtype == np.uint32 and rgba.shape == (height, width) and rgba.flags.c_contiguous
        rgb = np.empty((height, width, 3), dtype=np.float32) if want_rgb else None
        check(
            self._lib.rt_hip_render_progressive(
                self._ctx,
                C.byref(scene),
                rgba.ctypes.data,
                width,
                height,
                seed,
                flags,
                pass_samples,
                rgb.ctypes.data if rgb is not None else None,
                C.byref(stats_pod) if stats else None,
                C.byref(progress),
            )
        )
        self._progressive_size = (width, height)  # (the accumulation in flight: what denoise_progressive sizes its arrays by)
        return rgba, rgb, stats_pod.as_dict() if stats else {}, progress.as_dict()

    # ---- denoising --------------------------------------------------------------------------
    def guide_device(self, width: int, height: int, d_guide: int, flags: int = 0, stream: int | None = None) -> None:
        """rt_hip_guide_device: the first-hit guide of the resident scene (normal, depth | albedo, primitive id) into the DEVICE
        buffer `d_guide`, 8 floats per pixel.  Asynchronous on `stream`."""
        check(self._lib.rt_hip_guide_device(self._ctx, width, height, flags, d_guide, stream))

    def denoise_device(self, width: int, height: int, d_rgb_in: int, d_guide: int, params: RtHipDenoiseParams | None = None, d_rgb_out: int | None = None, d_rgba8_out: int | None = None, stream: int | None = None) -> None:
        """rt_hip_denoise_device: the edge-avoiding a-trous filter on DEVICE buffers (`params` None: the defaults).  Asynchronous."""
        check(self._lib.rt_hip_denoise_device(self._ctx, width, height, d_rgb_in, d_guide, C.byref(params) if params is not None else None, d_rgb_out, d_rgba8_out, stream))

    def denoise_progressive(self, params: RtHipDenoiseParams | None = None, want_rgb: bool = False, size: tuple | None = None):
        """rt_hip_denoise_progressive: the accumulation in flight of render_progressive, denoised — (rgba8 uint32[H, W], rgb
        float32[H, W, 3] or None, device milliseconds of guide + filter).  `size`: (width, height) of that accumulation (the
        frame render_progressive was last asked for); the accumulation itself is left alone."""
        width, height = size if size is not None else self._progressive_size
        rgba = np.empty((height, width), dtype=np.uint32)
        rgb = np.empty((height, width, 3), dtype=np.float32) if want_rgb else None
        ms = C.c_float()
        check(self._lib.rt_hip_denoise_progressive(self._ctx, C.byref(params) if params is not None else None, rgba.ctypes.data, rgb.ctypes.data if rgb is not None else None, C.byref(ms)))
        return rgba, rgb, ms.value

    # ---- temporal accumulation ---------------------------------------------------------------
    def reproject_device(self, width: int, height: int, prev_matrix, d_guide: int, d_rgb_in: int, samples_in: int, d_prev_rgb: int | None, d_prev_record: int | None, params: RtHipTemporalParams | None, d_rgb_out: int, d_record_out: int,
                         d_pixels_with_history: int | None = None, stream: int | None = None) -> None:
        """rt_hip_reproject_device: one reprojection step on DEVICE buffers; the current camera is the resident scene's, `prev_matrix`
        (16 floats, or None without a history) the one the history was made under.  Asynchronous on `stream`."""
        matrix = (C.c_float * 16)(*[float(v) for v in np.asarray(prev_matrix, dtype=np.float32).reshape(-1)]) if prev_matrix is not None else None
        check(self._lib.rt_hip_reproject_device(self._ctx, width, height, matrix, d_guide, d_rgb_in, samples_in, d_prev_rgb, d_prev_record, C.byref(params) if params is not None else None, d_rgb_out, d_record_out, d_pixels_with_history, stream))

    def render_temporal(self, scene: RtHipScene, width: int, height: int, seed: int = 1, flags: int = 0, temporal: RtHipTemporalParams | None = None, filter: RtHipDenoiseParams | None = None, want_rgb: bool = False, stats: bool = True):
        """rt_hip_render_temporal: one frame blended into the context's history — (rgba8 uint32[H, W], rgb float32[H, W, 3] or None,
        stats dict, info dict: frames, restarted, pixels_with_history, pixels).  Pass a new `seed` every frame.  `filter`: the
        a-trous filter's parameters for the delivered frame (None: no spatial filter)."""
        stats_pod, info = RtHipStats(), RtHipTemporalInfo()
        rgba = np.empty((height, width), dtype=np.uint32)
        rgb = np.empty((height, width, 3), dtype=np.float32) if want_rgb else None
        check(self._lib.rt_hip_render_temporal(self._ctx, C.byref(scene), rgba.ctypes.data, width, height, seed, flags, C.byref(temporal) if temporal is not None else None, C.byref(filter) if filter is not None else None,
                                               rgb.ctypes.data if rgb is not None else None, C.byref(stats_pod) if stats else None, C.byref(info)))
        return rgba, rgb, stats_pod.as_dict() if stats else {}, info.as_dict()

    # ---- guided upsampling ------------------------------------------------------------------
    def upsample_device(self, width: int, height: int, low_width: int, low_height: int, d_rgb_low: int, d_guide_low: int, d_guide_full: int, params: RtHipUpsampleParams | None = None, d_rgb_out: int | None = None,
                        d_rgba8_out: int | None = None, d_orphans: int | None = None, stream: int | None = None) -> None:
        """rt_hip_upsample_device: the full frame rebuilt from a low frame's mean and the guides of both sizes, on DEVICE buffers
        (`params` None: the defaults).  Asynchronous on `stream`."""
        check(self._lib.rt_hip_upsample_device(self._ctx, width, height, low_width, low_height, d_rgb_low, d_guide_low, d_guide_full, C.byref(params) if params is not None else None, d_rgb_out, d_rgba8_out, d_orphans, stream))

    def render_upscaled(self, scene: RtHipScene, width: int, height: int, seed: int = 1, flags: int = 0, factor: int = 2, upsample: RtHipUpsampleParams | None = None, filter: RtHipDenoiseParams | None = None, want_rgb: bool = False,
                        stats: bool = True):
        """rt_hip_render_upscaled: one frame traced at ceil(size / factor) and rebuilt at full size — (rgba8 uint32[H, W], rgb
        float32[H, W, 3] or None, stats dict of the traced low frame, info dict: low_width, low_height, orphans, pixels).  `filter`:
        the a-trous filter's parameters for the LOW mean (None: no filter)."""
        stats_pod, info = RtHipStats(), RtHipUpscaleInfo()
        rgba = np.empty((height, width), dtype=np.uint32)
        rgb = np.empty((height, width, 3), dtype=np.float32) if want_rgb else None
        check(self._lib.rt_hip_render_upscaled(self._ctx, C.byref(scene), rgba.ctypes.data, width, height, seed, flags, factor, C.byref(upsample) if upsample is not None else None, C.byref(filter) if filter is not None else None,
                                               rgb.ctypes.data if rgb is not None else None, C.byref(stats_pod) if stats else None, C.byref(info)))
        return rgba, rgb, stats_pod.as_dict() if stats else {}, info.as_dict()

    # ---- tone mapping ------------------------------------------------------------------------
    def tonemap_device(self, width: int, height: int, d_rgb_in: int, d_state: int, params: RtHipTonemapParams | None = None, d_rgb_out: int | None = None, d_rgba8_out: int | None = None, stream: int | None = None) -> None:
        """rt_hip_tonemap_device: a float frame on the DEVICE metered, exposed and mapped (`params` None: the defaults) into
        `d_rgb_out` (may be `d_rgb_in`) and / or `d_rgba8_out`; `d_state`: the caller's 8-word device record.  Asynchronous on `stream`."""
        check(self._lib.rt_hip_tonemap_device(self._ctx, width, height, d_rgb_in, C.byref(params) if params is not None else None, d_state, d_rgb_out, d_rgba8_out, stream))

    # ---- bloom -------------------------------------------------------------------------------
    def bloom_device(self, width: int, height: int, d_rgb_in: int, params: RtHipBloomParams | None = None, d_rgb_out: int | None = None, d_layer_out: int | None = None, stream: int | None = None) -> None:
        """rt_hip_bloom_device: a float frame on the DEVICE plus its glow (`params` None: the defaults) into `d_rgb_out` (may be
        `d_rgb_in`) and / or the glow layer alone into `d_layer_out`.  Asynchronous on `stream`."""
        check(self._lib.rt_hip_bloom_device(self._ctx, width, height, d_rgb_in, C.byref(params) if params is not None else None, d_rgb_out, d_layer_out, stream))

    def render_bloomed(self, scene: RtHipScene, width: int, height: int, seed: int = 1, flags: int = 0, bloom_params: RtHipBloomParams | None = None, tonemap_params: RtHipTonemapParams | None = None, want_rgb: bool = False,
                       stats: bool = True):
        """rt_hip_render_bloomed: one frame traced, bloomed, metered and tone-mapped on the device — (rgba8 uint32[H, W], the MAPPED rgb
        float32[H, W, 3] or None, stats dict of the traced frame, tone mapping's info dict)."""
        stats_pod, info = RtHipStats(), RtHipTonemapInfo()
        rgba = np.empty((height, width), dtype=np.uint32)
        rgb = np.empty((height, width, 3), dtype=np.float32) if want_rgb else None
        check(self._lib.rt_hip_render_bloomed(self._ctx, C.byref(scene), rgba.ctypes.data, width, height, seed, flags, C.byref(bloom_params) if bloom_params is not None else None,
                                              C.byref(tonemap_params) if tonemap_params is not None else None, rgb.ctypes.data if rgb is not None else None, C.byref(stats_pod) if stats else None, C.byref(info)))
        return rgba, rgb, stats_pod.as_dict() if stats else {}, info.as_dict()

    def render_tonemapped(self, scene: RtHipScene, width: int, height: int, seed: int = 1, flags: int = 0, params: RtHipTonemapParams | None = None, want_rgb: bool = False, stats: bool = True):
        """rt_hip_render_tonemapped: one frame traced, metered and tone-mapped on the device — (rgba8 uint32[H, W], the MAPPED rgb
        float32[H, W, 3] or None, stats dict of the traced frame, info dict: exposure, target, counted, skipped, kept, mean_q8)."""
        stats_pod, info = RtHipStats(), RtHipTonemapInfo()
        rgba = np.empty((height, width), dtype=np.uint32)
        rgb = np.empty((height, width, 3), dtype=np.float32) if want_rgb else None
        check(self._lib.rt_hip_render_tonemapped(self._ctx, C.byref(scene), rgba.ctypes.data, width, height, seed, flags, C.byref(params) if params is not None else None, rgb.ctypes.data if rgb is not None else None,
                                                 C.byref(stats_pod) if stats else None, C.byref(info)))
        return rgba, rgb, stats_pod.as_dict() if stats else {}, info.as_dict()

    # ---- adaptive sampling -----------------------------------------------------------------
    def render_adaptive(self, scene: RtHipScene, width: int, height: int, seed: int = 1, flags: int = 0, pass_samples: int = 16, params: RtHipAdaptiveParams | None = None, want_rgb: bool = False, want_counts: bool = True,
                        out: np.ndarray | None = None, stats: bool = True):
        """rt_hip_render_adaptive: the next pass of the adaptive accumulation in flight, over the pixels still active — or the first
        of a new one.  Returns (rgba8 uint32[H, W], rgb float32[H, W, 3] or None, sample map uint32[H, W] or None, stats dict of THIS
        pass, info dict: samples_done, samples_total, passes, restarted, active_pixels, pixels, samples_traced, complete).  Pixel
        (x, y) of the frame is the one-shot frame's pixel at samples_per_pixel = map[y, x], bit for bit."""
        stats_pod, info = RtHipStats(), RtHipAdaptiveInfo()
        rgba = out if out is not None else np.empty((height, width), dtype=np.uint32)
        assert rgba.dtype == np.uint32 and rgba.shape == (height, width) and rgba.flags.c_contiguous
        rgb = np.empty((height, width, 3), dtype=np.float32) if want_rgb else None
        counts = np.empty((height, width), dtype=np.uint32) if want_counts else None
        check(self._lib.rt_hip_render_adaptive(self._ctx, C.byref(scene), rgba.ctypes.data, width, height, seed, flags, pass_samples, C.byref(params) if params is not None else None, rgb.ctypes.data if rgb is not None else None,
                                               counts.ctypes.data if counts is not None else None, C.byref(stats_pod) if stats else None, C.byref(info)))
        return rgba, rgb, counts, stats_pod.as_dict() if stats else {}, info.as_dict()

    def adaptive_pass_device(self, width: int, height: int, first_sample: int, n_samples: int, d_block: int, d_rgba8: int, seed: int = 1, flags: int = 0, params: RtHipAdaptiveParams | None = None, d_rgb_f32: int | None = None,
                             d_active_pixels: int | None = None, stream: int | None = None) -> None:
        """rt_hip_adaptive_pass_device: one adaptive pass on the resident scene — samples [first_sample, first_sample + n_samples) of the
        active pixels, then the update step.  `d_block`: 9 x width x height words on the device (accum, state, pass_sum, moments)."""
        check(self._lib.rt_hip_adaptive_pass_device(self._ctx, width, height, seed, flags, first_sample, n_samples, C.byref(params) if params is not None else None, d_block, d_rgba8, d_rgb_f32, d_active_pixels, stream))

    def adaptive_update_device(self, width: int, height: int, pass_samples: int, first_pass: bool, whole_pass: bool, d_accum: int, d_pass_sum: int, d_moments: int, d_state: int, d_rgba8_out: int,
                               params: RtHipAdaptiveParams | None = None, d_rgb_out: int | None = None, d_active_pixels: int | None = None, stream: int | None = None) -> None:
        """rt_hip_adaptive_update_device: the update step alone on DEVICE buffers (moments and state in place).  Asynchronous."""
        check(self._lib.rt_hip_adaptive_update_device(self._ctx, width, height, pass_samples, int(bool(first_pass)), int(bool(whole_pass)), C.byref(params) if params is not None else None, d_accum, d_pass_sum, d_moments, d_state, d_rgba8_out,
                                                      d_rgb_out, d_active_pixels, stream))

    def forget_frame(self) -> None:
        """Drop the page-lock on the back buffer last rendered into with RT_HIP_FLAG_PERSISTENT_FRAME."""
        self._lib.rt_hip_forget_frame(self._ctx)

    def preview(self, scene: RtHipScene, width: int, height: int, want_rgb: bool = False, out: np.ndarray | None = None):
        """The one-ray-per-pixel preview (reference src/renderers/rasterizer.cpp) through the same drop-in call."""
        return self.render(scene, width, height, seed=0, flags=capi.RT_HIP_FLAG_PREVIEW, want_rgb=want_rgb, out=out)

    # ---- resident path ------------------------------------------------------------------------------------
    def upload(self, scene: RtHipScene) -> None:
        check(self._lib.rt_hip_scene_upload(self._ctx, C.byref(scene)))

    def render_device(
        self,
        width: int,
        height: int,
        d_rgba8: int,
        seed: int = 1,
        flags: int = 0,
        partition: tuple | None = None,
        d_rgb_f32: int | None = None,
        stream: int | None = None,
    ) -> None:
        part = C.byref(RtHipPartition(*partition)) if partition is not None else None
        check(self._lib.rt_hip_render_device(self._ctx, width, height, seed, flags, part, d_rgba8, d_rgb_f32, stream))

    def render_pass_device(
        self,
        width: int,
        height: int,
        first_sample: int,
        n_samples: int,
        d_accum: int,
        d_rgba8: int,
        seed: int = 1,
        flags: int = 0,
        partition: tuple | None = None,
        d_rgb_f32: int | None = None,
        stream: int | None = None,
    ) -> None:
        """rt_hip_render_pass_device: samples [first_sample, first_sample + n_samples) of the resident scene, folded onto the
        caller's accumulator `d_accum` (padded_local_rows x width x 3 floats on the device, kept from pass to pass)."""
        part = C.byref(RtHipPartition(*partition)) if partition is not None else None
        check(self._lib.rt_hip_render_pass_device(self._ctx, width, height, seed, flags, part, first_sample, n_samples, d_accum, d_rgba8, d_rgb_f32, stream))

    def assemble_device(self, width: int, height: int, world: int, stripe_rows: int, d_gathered: int, d_frame: int, stream: int | None = None) -> None:
        check(self._lib.rt_hip_assemble_device(self._ctx, width, height, world, stripe_rows, d_gathered, d_frame, stream))

    def stats(self) -> dict:
        stats = RtHipStats()
        check(self._lib.rt_hip_stats_fetch(self._ctx, C.byref(stats)))
        return stats.as_dict()

    def member_count(self) -> int:
        n = C.c_int()
        check(self._lib.rt_hip_member_count(self._ctx, C.byref(n)))
        return n.value

    def member_device(self, rank: int) -> int:
        d = C.c_int()
        check(self._lib.rt_hip_member_device(self._ctx, rank, C.byref(d)))
        return d.value

    def member_stats(self, rank: int) -> dict:
        """Counters of member `rank`'s share of the last render() on a multi-GPU tracer."""
        stats = RtHipStats()
        check(self._lib.rt_hip_member_stats(self._ctx, rank, C.byref(stats)))
        return stats.as_dict()

    # ---- known-answer entry points (librt_hip_kat.so: test-only, include/rt_hip_kat.h) ---------------------
    def kat_random(self, seed: int, pixel: int, sample: int, n: int) -> np.ndarray:
        out = np.empty(n, dtype=np.float32)
        capi.check_kat(capi.kat_lib().rt_hip_kat_random(self._ctx, seed, pixel, sample, n, out.ctypes.data))
        return out

    def kat_bvh_build_device(self) -> dict:
        """The sphere hierarchy RT_HIP_FLAG_BVH_DEVICE_BUILD builds for the resident scene, read back
        (rt_hip_kat_bvh_build_device): the dictionary of `bvh_build`, with one row of `nodes` per node SLOT."""
        counts = np.zeros(5, dtype=np.uint32)
        capi.check_kat(capi.kat_lib().rt_hip_kat_bvh_build_device(self._ctx, counts.ctypes.data, None, None, None, None, None))  # the sizes first
        n = max(int(counts[1]) + int(counts[2]), 1)
        nodes = np.zeros((n, 16), dtype=np.float32)
        order = np.zeros(n, dtype=np.uint32)
        spheres = np.zeros((n, 4), dtype=np.float32)
        always = np.zeros(n, dtype=np.uint32)
        bound = np.zeros(4, dtype=np.float32)
        capi.check_kat(capi.kat_lib().rt_hip_kat_bvh_build_device(self._ctx, counts.ctypes.data, nodes.ctypes.data, order.ctypes.data, spheres.ctypes.data, always.ctypes.data, bound.ctypes.data))
        n_nodes, n_tree, n_always, depth, root = (int(c) for c in counts)
        return {"nodes": nodes[:n_nodes], "order": order[:n_tree], "spheres": spheres[:n_tree], "always": always[:n_always], "bound": bound, "depth": depth, "root": root}

    def kat_box_bvh_builds(self) -> int:
        """How many box hierarchies (RT_HIP_FLAG_BOX_BVH) this context has built on the host so far (rt_hip_kat_box_bvh_builds)."""
        builds = C.c_uint64(0)
        capi.check_kat(capi.kat_lib().rt_hip_kat_box_bvh_builds(self._ctx, C.byref(builds)))
        return int(builds.value)

    def kat_closest_hit(self, origins: np.ndarray, directions: np.ndarray, bvh: bool = False, device_build: bool = False, boxes: bool = False, box_bvh: bool = False):
        """Closest hit of each ray against the resident scene: (distance, kind, index, normal).  `bvh`: through the sphere
        hierarchy of RT_HIP_FLAG_BVH (rt_hip_kat_closest_hit_bvh) instead of the linear scan; `device_build`: through the
        hierarchy the device builder makes (rt_hip_kat_closest_hit_bvh_device); `boxes`: RT_HIP_FLAG_TRACE_BOXES' query, the
        scene's boxes included (rt_hip_kat_closest_hit_boxes; kind 3 = box); `box_bvh`: the same with the boxes reached through
        RT_HIP_FLAG_BOX_BVH's hierarchy, any number of them (rt_hip_kat_closest_hit_boxes_bvh)."""
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(directions, dtype=np.float32).reshape(-1, 3)
        n = len(o)
        dist = np.empty(n, dtype=np.float32)
        kind = np.empty(n, dtype=np.uint32)
        index = np.empty(n, dtype=np.uint32)
        normal = np.empty((n, 3), dtype=np.float32)
        kat = capi.kat_lib()
        entry = kat.rt_hip_kat_closest_hit_bvh_device if device_build else (kat.rt_hip_kat_closest_hit_bvh if bvh else kat.rt_hip_kat_closest_hit)
        if boxes:
            entry = kat.rt_hip_kat_closest_hit_boxes
        if box_bvh:
            entry = kat.rt_hip_kat_closest_hit_boxes_bvh
        capi.check_kat(entry(self._ctx, n, o.ctypes.data, d.ctypes.data, dist.ctypes.data, kind.ctypes.data, index.ctypes.data, normal.ctypes.data))
        return dist, kind, index, normal

    def kat_sqrt_div(self, a: np.ndarray, b: np.ndarray):
        a = np.ascontiguousarray(a, dtype=np.float32)
        b = np.ascontiguousarray(b, dtype=np.float32)
        s = np.empty_like(a)
        q = np.empty_like(a)
        capi.check_kat(capi.kat_lib().rt_hip_kat_sqrt_div(self._ctx, a.size, a.ctypes.data, b.ctypes.data, s.ctypes.data, q.ctypes.data))
        return s, q

    def kat_fast_math(self, x: np.ndarray, y: np.ndarray):
        """RT_HIP_FLAG_FAST's leaf functions on the device, per element: (sqrt_rn(x), rcp_rn(x), inv_sqrt_rn(x), divide(x, y))."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        y = np.ascontiguousarray(y, dtype=np.float32)
        assert x.shape == y.shape
        out = [np.empty_like(x) for _ in range(4)]
        capi.check_kat(capi.kat_lib().rt_hip_kat_fast_math(self._ctx, x.size, x.ctypes.data, y.ctypes.data, *(o.ctypes.data for o in out)))
        return tuple(out)

    def kat_direct_octahedral(self, ka: np.ndarray, kb: np.ndarray) -> np.ndarray:
        """rt_amd/csrc/direct_light_rules.hpp's octahedral_point on the device: float32[n, 4] = (p.xyz, dot(p, p))."""
        ka = np.ascontiguousarray(ka, dtype=np.uint32)
        kb = np.ascontiguousarray(kb, dtype=np.uint32)
        out = np.empty((ka.size, 4), dtype=np.float32)
        capi.check_kat(capi.kat_lib().rt_hip_kat_direct_octahedral(self._ctx, ka.size, ka.ctypes.data, kb.ctypes.data, out.ctypes.data))
        return out

    def kat_direct_aim(self, ka: np.ndarray, kb: np.ndarray, vectors: np.ndarray, radius: np.ndarray, n_lights: int) -> np.ndarray:
        """... and its aim_at: vectors float32[n, 9] = (x, normal, centre) -> float32[n, 5] = (w.xyz, weight, aimed)."""
        ka = np.ascontiguousarray(ka, dtype=np.uint32)
        kb = np.ascontiguousarray(kb, dtype=np.uint32)
        vectors = np.ascontiguousarray(vectors, dtype=np.float32).reshape(ka.size, 9)
        radius = np.ascontiguousarray(radius, dtype=np.float32)
        out = np.empty((ka.size, 5), dtype=np.float32)
        capi.check_kat(capi.kat_lib().rt_hip_kat_direct_aim(self._ctx, ka.size, ka.ctypes.data, kb.ctypes.data, vectors.ctypes.data, radius.ctypes.data, n_lights, out.ctypes.data))
        return out

    def kat_lens(self, ka: np.ndarray, kb: np.ndarray, ray: np.ndarray, lens_words: np.ndarray) -> np.ndarray:
        """rt_amd/csrc/lens_rules.hpp on the device, as the lens builds run it: ray float32[9] = (origin, normalised direction, eye),
        lens_words float32[10] = (U, V, fwd, focus) -> float32[n, 9] = (lx, ly, origin, direction, bent)."""
        ka = np.ascontiguousarray(ka, dtype=np.uint32)
        kb = np.ascontiguousarray(kb, dtype=np.uint32)
        ray = np.ascontiguousarray(ray, dtype=np.float32).reshape(9)
        lens_words = np.ascontiguousarray(lens_words, dtype=np.float32).reshape(10)
        out = np.empty((ka.size, 9), dtype=np.float32)
        capi.check_kat(capi.kat_lib().rt_hip_kat_lens(self._ctx, ka.size, ka.ctypes.data, kb.ctypes.data, ray.ctypes.data, lens_words.ctypes.data, out.ctypes.data))
        return out

    def kat_exhaustive_math(self):
        """All 2^32 float bit patterns through the kernels' sqrt / reciprocal / reciprocal-sqrt sequences vs the
        compiler's correctly rounded expansions: ([mismatch counts], [first mismatching input bits])."""
        counts = (C.c_uint64 * 3)()
        first = (C.c_uint32 * 3)()
        capi.check_kat(capi.kat_lib().rt_hip_kat_exhaustive_math(self._ctx, C.byref(counts), C.byref(first)))
        return list(counts), list(first)
