"""tsdf_amd -- Python host mirror of the reference TSDF interface over the MI355X C ABI.

Reference interface mirrored (yuzhou42/disinfect-slam):
  * TSDFGrid            utils/tsdf/voxel_tsdf.cuh:32-124  (Integrate / RayCast / GatherValid /
                        GatherVoxels) -- here `TSDFGrid`, same argument meaning and order;
  * CameraIntrinsics    utils/cuda/camera.cuh:12-51, CameraParams :53-68
  * SE3                 utils/cuda/lie_group.cuh:6-45
  * BoundingCube        utils/tsdf/voxel_tsdf.cuh:12-27
  * VoxelSpatialTSDF    utils/tsdf/voxel_types.cuh:48-57 (numpy structured dtype VOXEL_DTYPE)
The C++17 facade (TSDFSystem / TSDFGrid / DISINFSystem TSDF methods) lives in ../host/.
Frames may be numpy arrays (host, copied by the engine) or torch CUDA tensors (device, no copy).
"""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np

from . import _lib
from ._lib import (SHARD_RECORD_BYTES, STATUS_DDA_OVERFLOW, STATUS_NEWKEY_OVERFLOW,
                   STATUS_PIPELINE_TIMEOUT, STATUS_POOL_EXHAUSTED, STATUS_SHARD_ABORTED, STATUS_SHARD_OVERFLOW, TSDF_MEM_DEVICE,
                   TSDF_MEM_HOST, TSDFError)

NUM_ENTRY = 1 << 22
NUM_BUCKET = 1 << 21
BLOCK_LEN = 8
BLOCK_VOLUME = 512
BLOCK_RECORD_BYTES = 16 + 12 * BLOCK_VOLUME  # TSDF_BLOCK_RECORD_BYTES: key header + block
# tsdf_component, 64 bytes: a cluster of Engine.components / Engine.frontiers
COMPONENT_DTYPE = np.dtype([("label", "<u4"), ("size", "<u4"), ("lo", "<i4", (3,)), ("hi", "<i4", (3,)),
                            ("sum", "<i8", (3,)), ("goal", "<u4"), ("goal_key", "<u4")])
TSDF_COMPONENT_NONE = 0xFFFFFFFF
# Engine.view_gain takes its views this many at a time (TSDF_VIEW_BATCH), fewer while a batch's pixels exceed 2^22
VIEW_BATCH = 64
VOXEL_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("tsdf", "<f4")])

__all__ = [
    "CameraIntrinsics", "CameraParams", "SE3", "BoundingCube", "TSDFGrid", "Engine", "ShardGroup",
    "VOXEL_DTYPE", "TSDFError", "hash_block", "block_owner", "load_library", "FOREIGN_IDX",
    "STATUS_SHARD_ABORTED",
    "STATUS_PIPELINE_TIMEOUT",
]
FOREIGN_IDX = 0x7FFFFFFF  # a shard's index entry of a block another shard holds (kForeignIdx)


def load_library():
    return _lib.load()


def hash_block(x: int, y: int, z: int) -> int:
    """voxel_hash.cu:31-35 Hash."""
    return int(_lib.load().tsdf_hash_block(x, y, z))


def block_owner(x: int, y: int, z: int, shard_count: int) -> int:
    return int(_lib.load().tsdf_block_owner(x, y, z, shard_count))


@dataclasses.dataclass(frozen=True)
class CameraIntrinsics:
    """camera.cuh:12-51 CameraIntrinsics<float>."""
    fx: float
    fy: float
    cx: float
    cy: float

    def Inverse(self) -> "CameraIntrinsics":
        f32 = np.float32
        fx_inv = f32(1) / f32(self.fx)
        fy_inv = f32(1) / f32(self.fy)
        return CameraIntrinsics(float(fx_inv), float(fy_inv), float(-f32(self.cx) * fx_inv),
                                float(-f32(self.cy) * fy_inv))

    def _c(self) -> _lib.Intrinsics:
        c = self.__dict__.get("_cc")
        if c is None:  # frozen dataclass: cache the ctypes struct once
            c = _lib.Intrinsics(self.fx, self.fy, self.cx, self.cy)
            object.__setattr__(self, "_cc", c)
        return c


@dataclasses.dataclass(frozen=True)
class CameraParams:
    """camera.cuh:53-68 CameraParams(intrinsics, img_h, img_w)."""
    intrinsics: CameraIntrinsics
    img_h: int
    img_w: int


def _qmul_sse(a, b):
    """Eigen quat_product<SSE, float> (host Eigen, Geometry/arch/Geometry_SSE.h)."""
    f32 = np.float32
    a0, a1, a2, a3 = (f32(v) for v in a)
    b0, b1, b2, b3 = (f32(v) for v in b)
    x = (a0 * b3 - a2 * b1) + (a1 * b2 + a3 * b0)
    y = (a1 * b3 - a0 * b2) + (a2 * b0 + a3 * b1)
    z = (a2 * b3 - a1 * b0) + (a0 * b1 + a3 * b2)
    w = (a3 * b3 - a0 * b0) - (a2 * b2 + a1 * b1)
    return np.array([x, y, z, w], np.float32)


def _qrot(q, v):
    """Eigen QuaternionBase::_transformVector."""
    f32 = np.float32
    qx, qy, qz, qw = (f32(c) for c in q)
    vx, vy, vz = (f32(c) for c in v)
    ux = qy * vz - qz * vy
    uy = qz * vx - qx * vz
    uz = qx * vy - qy * vx
    ux, uy, uz = ux + ux, uy + uy, uz + uz
    cx = qy * uz - qz * uy
    cy = qz * ux - qx * uz
    cz = qx * uy - qy * ux
    return np.array([(vx + qw * ux) + cx, (vy + qw * uy) + cy, (vz + qw * uz) + cz], np.float32)


class SE3:
    """lie_group.cuh:6-45 SE3<float>: rotation quaternion (x, y, z, w) + translation."""

    def __init__(self, q_xyzw=(0.0, 0.0, 0.0, 1.0), t=(0.0, 0.0, 0.0)):
        self.q = np.asarray(q_xyzw, dtype=np.float32).reshape(4).copy()
        self.t = np.asarray(t, dtype=np.float32).reshape(3).copy()

    @staticmethod
    def Identity() -> "SE3":
        return SE3()

    def GetR(self):
        return self.q.copy()

    def GetT(self):
        return self.t.copy()

    def Inverse(self) -> "SE3":
        f32 = np.float32
        x, y, z, w = (f32(c) for c in self.q)
        n2 = (x * x + z * z) + (y * y + w * w)
        qi = np.array([-x / n2, -y / n2, -z / n2, w / n2], np.float32) if n2 > 0 else np.zeros(4, np.float32)
        return SE3(qi, _qrot(qi, -self.t))

    def Apply(self, v):
        return (_qrot(self.q, v) + self.t).astype(np.float32)

    def __mul__(self, other: "SE3") -> "SE3":
        return SE3(_qmul_sse(self.q, other.q), _qrot(self.q, other.t) + self.t)

    def _c(self) -> _lib.Pose:
        c = self.__dict__.get("_cc")
        if c is None:  # SE3 is treated as immutable: cache the ctypes struct once
            c = _lib.Pose(*[float(v) for v in self.q], *[float(v) for v in self.t])
            self._cc = c
        return c


@dataclasses.dataclass(frozen=True)
class BoundingCube:
    """voxel_tsdf.cuh:12-27 BoundingCube<float>."""
    xmin: float
    xmax: float
    ymin: float
    ymax: float
    zmin: float
    zmax: float

    def as_array(self):
        return np.array([self.xmin, self.xmax, self.ymin, self.ymax, self.zmin, self.zmax], np.float32)


def _is_torch_cuda(x) -> bool:
    return hasattr(x, "data_ptr") and hasattr(x, "is_cuda") and bool(x.is_cuda)


_raw_stream = None


def _current_raw_stream(device: int) -> int:
    """torch's current stream on `device` as a raw hipStream_t (the cheap accessor when this torch has
    it: torch.cuda.current_stream() builds a Stream object per call)."""
    global _raw_stream
    if _raw_stream is None:
        import torch
        f = getattr(torch._C, "_cuda_getCurrentRawStream", None)
        _raw_stream = f if f is not None else (lambda d: torch.cuda.current_stream(d).cuda_stream)
    return int(_raw_stream(device) or 0)


def _ptr(x):
    if x is None:
        return None
    if _is_torch_cuda(x):
        return C.c_void_p(x.data_ptr())
    return x.ctypes.data_as(C.c_void_p)


def _np(a, dtype):
    return None if a is None else np.ascontiguousarray(a, dtype=dtype)



class FrameGraph:
    """One instantiated per-frame hipGraph of an Engine (tsdf_graph_create). frame() takes device
    tensors only; rgba / normal are device tensors (render_height, render_width, 4) u8 or None."""

    def __init__(self, eng, width, height, render_width=0, render_height=0, deferred=False, batch=1):
        self._eng = eng
        self.width, self.height = width, height
        self.render_width, self.render_height = render_width, render_height
        h = C.c_void_p()
        if batch > 1:  # tsdf_graph_create_batch: `batch` frames per graph launch
            _lib.check(_lib.load().tsdf_graph_create_batch(eng._h, width, height, render_width, render_height,
                                                           int(deferred), batch, C.byref(h)), "tsdf_graph_create_batch")
        else:
            fn = "tsdf_graph_create_deferred" if deferred else "tsdf_graph_create"
            _lib.check(getattr(_lib.load(), fn)(eng._h, width, height, render_width, render_height, C.byref(h)), fn)
        self.batch = batch
        self._g = h
        self.deferred = deferred

    def frame(self, rgb, depth, ht, lt, K, cam_T_world, max_depth, render_K=None,
              render_cam_T_world=None, rgba=None, normal=None):
        for a in (rgb, depth, ht, lt, rgba, normal):
            if a is not None and (not _is_torch_cuda(a) or not a.is_contiguous()):
                raise ValueError("graph frames take contiguous device tensors")
        H, W = int(depth.shape[0]), int(depth.shape[1])
        fr = _lib.Frame(W, H, _ptr(rgb), _ptr(depth), _ptr(ht), _ptr(lt), TSDF_MEM_DEVICE)
        Kc = K._c() if isinstance(K, CameraIntrinsics) else _lib.Intrinsics(*[float(v) for v in K])
        Rk = None
        if render_K is not None:
            Rk = render_K._c() if isinstance(render_K, CameraIntrinsics) else \
                _lib.Intrinsics(*[float(v) for v in render_K])
        self._eng._wait_torch(depth)
        prev = self._eng._pending
        _lib.check(_lib.load().tsdf_graph_frame(
            self._g, C.byref(fr), C.byref(Kc), C.byref(cam_T_world._c()), max_depth,
            C.byref(Rk) if Rk is not None else None,
            C.byref(render_cam_T_world._c()) if render_cam_T_world is not None else None,
            _ptr(rgba), _ptr(normal)), "tsdf_graph_frame")
        self._eng._signal_torch(depth)
        if self.batch > 1:
            # a batched graph writes a frame's images when its batch launches (full, or at the engine's
            # next other call): every image of the unlaunched frames stays referenced until such a call
            if rgba is not None or normal is not None:
                self._eng._pending = (prev or ()) + (rgba, normal)
            return
        self._eng._after_call(prev)
        if self.deferred and (rgba is not None or normal is not None):
            self._eng._pending = (rgba, normal)  # written by the next launch (or engine call)

    def close(self):
        if getattr(self, "_g", None):
            _lib.load().tsdf_graph_destroy(self._g)
            self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

class ShardFrameGraph:
    """A shard engine's graph-captured sharded frame (tsdf_graph_create_shard): begin / update / end
    as three graph launches around the caller's two exchanges. Device frames and device slots."""

    def __init__(self, eng, width, height, slice_index=0, slice_count=1):
        self._eng = eng
        self.width, self.height = width, height
        self.split = slice_count > 1
        h = C.c_void_p()
        _lib.check(_lib.load().tsdf_graph_create_shard(eng._h, width, height, slice_index, slice_count,
                                                       C.byref(h)), "tsdf_graph_create_shard")
        self._g = h

    def begin(self, rgb, depth, ht, lt, K, cam_T_world, max_depth, keys_out, keys_in, key_cap, cands_out,
              cands_in, cand_cap):
        for a in (rgb, depth, ht, lt, keys_out, keys_in, cands_out, cands_in):
            if a is not None and (not _is_torch_cuda(a) or not a.is_contiguous()):
                raise ValueError("shard graph frames take contiguous device tensors")
        H, W = int(depth.shape[0]), int(depth.shape[1])
        fr = _lib.Frame(W, H, _ptr(rgb), _ptr(depth), _ptr(ht), _ptr(lt), TSDF_MEM_DEVICE)
        Kc = K._c() if isinstance(K, CameraIntrinsics) else _lib.Intrinsics(*[float(v) for v in K])
        self._eng._wait_torch(depth, keys_out, cands_out)
        _lib.check(_lib.load().tsdf_graph_shard_begin(
            self._g, C.byref(fr), C.byref(Kc), C.byref(cam_T_world._c()), max_depth, _ptr(keys_out),
            _ptr(keys_in), key_cap, _ptr(cands_out), _ptr(cands_in), cand_cap), "tsdf_graph_shard_begin")
        self._eng._signal_torch(keys_out)
        self._frame = (rgb, depth, ht, lt)  # read again by the update segment (see Engine.integrate_shard_begin)

    def update(self, keys_in=None, cands_out=None):
        self._eng._wait_torch(keys_in)
        _lib.check(_lib.load().tsdf_graph_shard_update(self._g), "tsdf_graph_shard_update")
        keep, self._frame = getattr(self, "_frame", None) or (), None
        self._eng._signal_torch(cands_out, *keep)

    def end(self, cands_in=None):
        self._eng._wait_torch(cands_in)
        _lib.check(_lib.load().tsdf_graph_shard_end(self._g), "tsdf_graph_shard_end")
        self._eng._signal_torch(cands_in)

    def close(self):
        if getattr(self, "_g", None):
            _lib.load().tsdf_graph_destroy(self._g)
            self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Engine:
    """One MI355X TSDF volume (one GPU shard). Thin owner of a tsdf_engine* handle."""

    def __init__(self, voxel_size=0.005, truncation=0.03, max_width=1920, max_height=1080,
                 num_block_bits=18, device=0, shard_index=0, shard_count=1, stream=None):
        L = _lib.load()
        cfg = _lib.Config()
        L.tsdf_config_default(C.byref(cfg))
        cfg.voxel_size = voxel_size
        cfg.truncation = truncation
        cfg.max_width = max_width
        cfg.max_height = max_height
        cfg.num_block_bits = num_block_bits
        cfg.shard_index = shard_index
        cfg.shard_count = shard_count
        if stream is not None:  # a torch.cuda.Stream or a raw hipStream_t (0 = the legacy default stream)
            cfg.stream = C.c_void_p(int(getattr(stream, "cuda_stream", getattr(stream, "value", stream)) or 0))
            cfg.use_stream = 1
        h = C.c_void_p()
        _lib.check(L.tsdf_create(C.byref(cfg), device, C.byref(h)), "tsdf_create")
        self._h = h
        # the engine orders its stream after / before torch's current stream around every call that
        # reads / writes a torch device tensor (tsdf_stream_wait / _signal) whenever the two differ
        # (an engine-owned stream, or a caller's stream other than torch's current one)
        es = C.c_void_p()
        _lib.check(L.tsdf_get_stream(h, C.byref(es)), "tsdf_get_stream")
        self._stream = int(es.value or 0)
        self.voxel_size = voxel_size
        self.truncation = truncation
        self.num_blocks = int(L.tsdf_num_blocks(h))
        self.device = device
        self.shard_index = shard_index
        self.shard_count = shard_count
        # device images of a deferred raycast (raycast(deferred=True), deferred graph frames) that the
        # engine's NEXT call writes: referenced until then (torch's allocator must not reuse them), and
        # torch's current stream is ordered after that call -- see _after_call
        self._pending = None
        # extract_mesh_indexed(device=True): vertex / triangle capacities of its first attempt
        self._mesh_caps = (1 << 16, 1 << 17)

    def _after_call(self, prev):
        """Engine call wrapper epilogue: the call launched the deferred raycast `prev` was waiting for
        (every engine entry point does, tsdf_raycast_deferred included), so torch's current stream now
        waits for the engine's queued work -- the images may be read there -- and the reference goes."""
        if prev is None:
            return
        if self._pending is prev:
            self._pending = None
        self._signal_torch(*(t for t in prev if t is not None))

    def close(self):
        self._pending = None
        if getattr(self, "_h", None):
            _lib.load().tsdf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- hot path ----
    def _frame(self, rgb, depth, ht, lt):
        dev = _is_torch_cuda(depth)
        if dev:
            H, W = int(depth.shape[0]), int(depth.shape[1])
            for a in (rgb, depth, ht, lt):
                if a is not None and not a.is_contiguous():
                    raise ValueError("device frames must be contiguous")
        else:
            rgb = _np(rgb, np.uint8)
            depth = _np(depth, np.float32)
            ht = _np(ht, np.float32)
            lt = _np(lt, np.float32)
            H, W = depth.shape
        if tuple(rgb.shape[:2]) != (H, W):
            raise ValueError("rgb / depth size mismatch (voxel_tsdf.cu:352-353)")
        # the arrays stay referenced by the caller for the duration of the call
        return _lib.Frame(W, H, _ptr(rgb), _ptr(depth), _ptr(ht), _ptr(lt),
                          TSDF_MEM_DEVICE if dev else TSDF_MEM_HOST), (rgb, depth, ht, lt)

    def _rgbd_inputs(self, rgb, depth_u16, mask):
        dev = _is_torch_cuda(depth_u16)
        if dev:
            for a in (rgb, depth_u16, mask):
                if a is not None and not a.is_contiguous():
                    raise ValueError("device frames must be contiguous")
        else:
            rgb = _np(rgb, np.uint8)
            depth_u16 = _np(depth_u16, np.uint16)
            mask = _np(mask, np.uint8)
        H, W = int(depth_u16.shape[0]), int(depth_u16.shape[1])
        if tuple(rgb.shape[:2]) != (H, W) or (mask is not None and tuple(mask.shape[:2]) != (H, W)):
            raise ValueError("rgb / depth / mask size mismatch")
        return dev, rgb, depth_u16, mask, W, H

    def rgbd_half(self, rgb, depth_u16, mask, depth_factor: float):
        """DISINFSystem::feed_rgbd_frame preprocessing alone (x0.5 resize, depth scale, mask):
        returns (rgb (H/2, W/2, 3) u8, depth (H/2, W/2) f32), host arrays or device tensors."""
        dev, rgb, depth_u16, mask, W, H = self._rgbd_inputs(rgb, depth_u16, mask)
        if dev:
            import torch
            ro = torch.empty((H // 2, W // 2, 3), dtype=torch.uint8, device=depth_u16.device)
            do = torch.empty((H // 2, W // 2), dtype=torch.float32, device=depth_u16.device)
        else:
            ro = np.zeros((H // 2, W // 2, 3), np.uint8)
            do = np.zeros((H // 2, W // 2), np.float32)
        self._wait_torch(depth_u16, ro)
        _lib.check(_lib.load().tsdf_rgbd_half(self._h, _ptr(rgb), _ptr(depth_u16), _ptr(mask), W, H,
                                              depth_factor, _ptr(ro), _ptr(do),
                                              TSDF_MEM_DEVICE if dev else TSDF_MEM_HOST), "tsdf_rgbd_half")
        self._signal_torch(depth_u16, ro)
        return ro, do

    def feed_rgbd_frame(self, rgb, depth_u16, mask, depth_factor: float, K, cam_T_world: SE3,
                        max_depth: float):
        """DISINFSystem::feed_rgbd_frame after its pose lookup: preprocessing + Integrate on the GPU
        (K = intrinsics of the half-size image)."""
        dev, rgb, depth_u16, mask, W, H = self._rgbd_inputs(rgb, depth_u16, mask)
        Kc = K._c() if isinstance(K, CameraIntrinsics) else _lib.Intrinsics(*[float(v) for v in K])
        self._wait_torch(depth_u16)
        _lib.check(_lib.load().tsdf_feed_rgbd_frame(self._h, _ptr(rgb), _ptr(depth_u16), _ptr(mask), W, H,
                                                    depth_factor, C.byref(Kc), C.byref(cam_T_world._c()),
                                                    max_depth, TSDF_MEM_DEVICE if dev else TSDF_MEM_HOST),
                   "tsdf_feed_rgbd_frame")
        self._signal_torch(depth_u16)

    def frame_graph(self, width: int, height: int, render_width: int = 0, render_height: int = 0,
                    deferred: bool = False, batch: int = 1):
        """Graph-captured frame loop (tsdf_graph_*, BASELINE config C5): integrate (+ raycast of
        a render camera) as one hipGraph launch per frame. deferred=True (tsdf_graph_create_deferred):
        each frame's images are written by the next frame's launch (or the engine's next other call)."""
        return FrameGraph(self, width, height, render_width, render_height, deferred, batch)

    def shard_frame_graph(self, width: int, height: int, slice_index: int = 0, slice_count: int = 1):
        """A shard's graph-captured sharded frame (tsdf_graph_create_shard)."""
        return ShardFrameGraph(self, width, height, slice_index, slice_count)

    # ---- stream ordering with torch (device tensors on torch's current stream) ----
    def _torch_stream(self, tensors):
        """torch's current stream when it differs from the engine stream and a device tensor is
        involved, else None (same stream: already ordered)."""
        if not any(_is_torch_cuda(t) for t in tensors if t is not None):
            return None
        import torch
        cur = _current_raw_stream(torch.cuda.current_device())
        return None if cur == self._stream else cur

    def _wait_torch(self, *tensors):
        """Engine stream waits for torch's current stream when a device tensor goes in."""
        cur = self._torch_stream(tensors)
        if cur is not None:
            _lib.check(_lib.load().tsdf_stream_wait(self._h, C.c_void_p(cur)), "tsdf_stream_wait")

    def _signal_torch(self, *tensors):
        """Torch's current stream waits for the engine when a device tensor it wrote / reads is
        handed back (or may be freed by the caller)."""
        cur = self._torch_stream(tensors)
        if cur is not None:
            _lib.check(_lib.load().tsdf_stream_signal(self._h, C.c_void_p(cur)), "tsdf_stream_signal")

    # ---- sharded frames (tsdf_integrate_shard_*) ----
    @staticmethod
    def shard_slot_bytes(cap: int) -> int:
        """Bytes of one exchange slot: cap records + the count header (tsdf_shard_slot_bytes)."""
        return int(_lib.load().tsdf_shard_slot_bytes(cap))

    def _check_slot(self, buf, cap, slots, what):
        if not _is_torch_cuda(buf) or not buf.is_contiguous() or \
                buf.numel() * buf.element_size() < slots * self.shard_slot_bytes(cap):
            raise ValueError(f"{what} must be a contiguous device tensor of {slots} x shard_slot_bytes({cap})")

    def integrate_shard_begin(self, rgb, depth, ht, lt, K, cam_T_world: SE3, max_depth: float,
                              slice_index: int = 0, slice_count: int = 1, keys_out=None, key_cap: int = 0):
        """Sharded frame, phase 1: pixel records, visibility of this shard's blocks, and the DDA over
        slice `slice_index` of `slice_count` (tile-row bands); the keys it finds go to keys_out (one
        slot), or stay here when slice_count == 1 and keys_out is None (every shard runs the whole
        DDA)."""
        if keys_out is not None:
            self._check_slot(keys_out, key_cap, 1, "keys_out")
        fr, keep = self._frame(rgb, depth, ht, lt)
        self._wait_torch(depth, keys_out)
        Kc = K._c() if isinstance(K, CameraIntrinsics) else _lib.Intrinsics(*[float(v) for v in K])
        _lib.check(_lib.load().tsdf_integrate_shard_begin(self._h, C.byref(fr), C.byref(Kc),
                                                          C.byref(cam_T_world._c()), max_depth,
                                                          slice_index, slice_count, _ptr(keys_out),
                                                          key_cap), "tsdf_integrate_shard_begin")
        self._signal_torch(keys_out)
        # the update (_update) gathers the raw device frame again: the tensors stay referenced here
        # (a temporary such as depth.float() is not freed and reused by torch's allocator) and torch's
        # stream is ordered after the engine for them only once _update is enqueued
        self._shard_frame = keep if _is_torch_cuda(depth) else None

    def integrate_shard_update(self, keys_in, key_cap: int, cands_out, cand_cap: int):
        """Sharded frame, phase 2: merge the all-gathered key slots (None after a whole-frame DDA),
        allocate, update this shard's blocks, write its carve candidates to cands_out (one slot)."""
        if keys_in is not None:
            self._check_slot(keys_in, key_cap, self.shard_count, "keys_in")
        self._check_slot(cands_out, cand_cap, 1, "cands_out")
        self._wait_torch(keys_in, cands_out)
        _lib.check(_lib.load().tsdf_integrate_shard_update(self._h, _ptr(keys_in), key_cap, _ptr(cands_out),
                                                           cand_cap), "tsdf_integrate_shard_update")
        self._release_shard_frame(keys_in, cands_out)

    def _release_shard_frame(self, *tensors):
        """The engine no longer reads the sharded frame's raw tensors once its update is enqueued:
        torch's stream waits for the engine, then the references go."""
        keep = getattr(self, "_shard_frame", None) or ()
        self._signal_torch(*tensors, *keep)
        self._shard_frame = None

    def integrate_shard_end(self, cands_in, cand_cap: int):
        """Sharded frame, phase 3: delete the all-gathered carve candidates (every shard's)."""
        self._check_slot(cands_in, cand_cap, self.shard_count, "cands_in")
        self._wait_torch(cands_in)
        _lib.check(_lib.load().tsdf_integrate_shard_end(self._h, _ptr(cands_in), cand_cap),
                   "tsdf_integrate_shard_end")
        self._signal_torch(cands_in)

    def integrate_shard_pipe(self, rgb, depth, ht, lt, K, cam_T_world, max_depth: float, cands_in, cands_out,
                             cand_cap: int) -> bool:
        """Pipelined sharded frame, one exchange per frame (tsdf_integrate_shard_pipe): this frame's
        ingest (the whole frame's DDA on every shard), the previous frame's allocation and update (this
        shard's carve candidates into cands_out, one slot), the frame before's carving of every shard's
        candidates (cands_in: the all-gathered slots of the previous call). depth None: one step of
        completing the pending frames. Returns True while more such steps (each after an exchange)
        are needed."""
        self._check_slot(cands_out, cand_cap, 1, "cands_out")
        self._check_slot(cands_in, cand_cap, self.shard_count, "cands_in")
        pend = C.c_int32(0)
        if depth is None:
            self._wait_torch(cands_in, cands_out)
            _lib.check(_lib.load().tsdf_integrate_shard_pipe(self._h, None, None, None, max_depth, _ptr(cands_in),
                                                             _ptr(cands_out), cand_cap, C.byref(pend)),
                       "tsdf_integrate_shard_pipe")
            self._signal_torch(cands_in, cands_out)
            return bool(pend.value)
        fr, keep = self._frame(rgb, depth, ht, lt)
        Kc = K._c() if isinstance(K, CameraIntrinsics) else _lib.Intrinsics(*[float(v) for v in K])
        self._wait_torch(depth, cands_in, cands_out)
        _lib.check(_lib.load().tsdf_integrate_shard_pipe(self._h, C.byref(fr), C.byref(Kc), C.byref(cam_T_world._c()),
                                                         max_depth, _ptr(cands_in), _ptr(cands_out), cand_cap,
                                                         C.byref(pend)), "tsdf_integrate_shard_pipe")
        self._signal_torch(depth, cands_in, cands_out)  # (the frame is read by this call only)
        del keep
        return bool(pend.value)

    def integrate_shard_abort(self):
        """Abort a pending sharded frame (tsdf_integrate_shard_abort): the engine is between frames
        again; STATUS_SHARD_ABORTED is set because shards may have diverged (restore snapshots)."""
        try:
            _lib.check(_lib.load().tsdf_integrate_shard_abort(self._h), "tsdf_integrate_shard_abort")
        finally:
            self._release_shard_frame()

    def integrate(self, rgb, depth, ht, lt, K, cam_T_world: SE3, max_depth: float):
        dev = getattr(depth, "is_cuda", False) is True and hasattr(depth, "data_ptr")
        if dev:  # (the hot path: torch's stream is looked up once, no extra ordering calls when the
            # engine runs on it; ctypes passes the structs by reference itself)
            H, W = depth.shape[0], depth.shape[1]
            if not (rgb.is_contiguous() and depth.is_contiguous() and (ht is None or ht.is_contiguous())
                    and (lt is None or lt.is_contiguous())):
                raise ValueError("device frames must be contiguous")
            if rgb.shape[0] != H or rgb.shape[1] != W:
                raise ValueError("rgb / depth size mismatch (voxel_tsdf.cu:352-353)")
            fr = _lib.Frame(W, H, rgb.data_ptr(), depth.data_ptr(), ht.data_ptr() if ht is not None else None,
                            lt.data_ptr() if lt is not None else None, TSDF_MEM_DEVICE)
            Kc = K._c() if isinstance(K, CameraIntrinsics) else _lib.Intrinsics(*[float(v) for v in K])
            cur = _current_raw_stream(depth.get_device())
            L = _lib.load()
            if cur != self._stream:
                _lib.check(L.tsdf_stream_wait(self._h, C.c_void_p(cur)), "tsdf_stream_wait")
            rc = L.tsdf_integrate(self._h, fr, Kc, cam_T_world._c(), max_depth)
            if rc:
                _lib.check(rc, "tsdf_integrate")
            if cur != self._stream:
                _lib.check(L.tsdf_stream_signal(self._h, C.c_void_p(cur)), "tsdf_stream_signal")
            return
        else:
            rgb = _np(rgb, np.uint8)
            depth = _np(depth, np.float32)
            ht = _np(ht, np.float32)
            lt = _np(lt, np.float32)
            H, W = depth.shape
        if tuple(rgb.shape[:2]) != (H, W):
            raise ValueError("rgb / depth size mismatch (voxel_tsdf.cu:352-353)")
        fr = _lib.Frame(W, H, _ptr(rgb), _ptr(depth), _ptr(ht), _ptr(lt),
                        TSDF_MEM_DEVICE if dev else TSDF_MEM_HOST)
        Kc = K._c() if isinstance(K, CameraIntrinsics) else _lib.Intrinsics(*[float(v) for v in K])
        self._wait_torch(depth)
        _lib.check(_lib.load().tsdf_integrate(self._h, C.byref(fr), C.byref(Kc),
                                              C.byref(cam_T_world._c()), max_depth),
                   "tsdf_integrate")
        self._signal_torch(depth)  # the caller may overwrite / free the frame after this

    def synchronize(self):
        _lib.check(_lib.load().tsdf_synchronize(self._h), "tsdf_synchronize")

    def flush(self):
        """Enqueue the deferred update of the last integrated frame (pipelined frames) on the engine
        stream without waiting: a device synchronisation (torch.cuda.synchronize) afterwards covers
        every frame integrated so far."""
        _lib.check(_lib.load().tsdf_flush(self._h), "tsdf_flush")

    # ---- extraction ----
    def raycast(self, K, width, height, cam_T_world: SE3, max_depth: float, rgba=None, normal=None,
                deferred=False):
        """tsdf_raycast; deferred=True (device tensors only): tsdf_raycast_deferred -- the images are
        written by the engine's next call (fused with the next frame's ingest when that is integrate;
        flush() otherwise); after that call they may be read on torch's current stream (the engine keeps
        them referenced until then and orders torch's stream after the call)."""
        Kc = K._c() if isinstance(K, CameraIntrinsics) else _lib.Intrinsics(*[float(v) for v in K])
        if deferred:
            if rgba is None or not _is_torch_cuda(rgba) or (normal is not None and not _is_torch_cuda(normal)):
                raise ValueError("a deferred raycast writes device tensors")
            self._wait_torch(rgba, normal)
            _lib.check(_lib.load().tsdf_raycast_deferred(self._h, C.byref(Kc), width, height,
                                                         C.byref(cam_T_world._c()), max_depth, _ptr(rgba),
                                                         _ptr(normal)), "tsdf_raycast_deferred")
            self._pending = (rgba, normal)
            return rgba, normal
        if rgba is not None and _is_torch_cuda(rgba):
            self._wait_torch(rgba, normal)
            _lib.check(_lib.load().tsdf_raycast(self._h, C.byref(Kc), width, height,
                                                C.byref(cam_T_world._c()), max_depth, _ptr(rgba),
                                                _ptr(normal), TSDF_MEM_DEVICE), "tsdf_raycast")
            self._signal_torch(rgba, normal)
            return rgba, normal
        rgba = np.zeros((height, width, 4), np.uint8)
        normal = np.zeros((height, width, 4), np.uint8)
        _lib.check(_lib.load().tsdf_raycast(self._h, C.byref(Kc), width, height,
                                            C.byref(cam_T_world._c()), max_depth, _ptr(rgba),
                                            _ptr(normal), TSDF_MEM_HOST), "tsdf_raycast")
        return rgba, normal

    def raycast_rows(self, K, width, height, cam_T_world: SE3, max_depth: float, row0: int, nrows: int,
                     rgba=None, normal=None):
        """Rows [row0, row0 + nrows) of raycast(K, width, height, ...) (tsdf_raycast_rows): numpy
        (nrows, width, 4) u8 images, or into the given device tensors."""
        Kc = K._c() if isinstance(K, CameraIntrinsics) else _lib.Intrinsics(*[float(v) for v in K])
        if rgba is not None and _is_torch_cuda(rgba):
            self._wait_torch(rgba, normal)
            _lib.check(_lib.load().tsdf_raycast_rows(self._h, C.byref(Kc), width, height,
                                                     C.byref(cam_T_world._c()), max_depth, row0, nrows,
                                                     _ptr(rgba), _ptr(normal), TSDF_MEM_DEVICE), "tsdf_raycast_rows")
            self._signal_torch(rgba, normal)
            return rgba, normal
        rgba = np.zeros((nrows, width, 4), np.uint8)
        normal = np.zeros((nrows, width, 4), np.uint8)
        _lib.check(_lib.load().tsdf_raycast_rows(self._h, C.byref(Kc), width, height, C.byref(cam_T_world._c()),
                                                 max_depth, row0, nrows, _ptr(rgba), _ptr(normal), TSDF_MEM_HOST),
                   "tsdf_raycast_rows")
        return rgba, normal

    def _grouped(self, fn, args, ngroups, device):
        """Two-call grouped records (tsdf_render_bands / tsdf_pack_halo) -> (counts, records)."""
        counts = np.zeros(ngroups, np.int64)
        _lib.check(fn(*args, None, 0, _ptr(counts), TSDF_MEM_HOST), fn.__name__)
        n = int(counts.sum())
        if device:
            import torch
            out = torch.empty((n, BLOCK_RECORD_BYTES), dtype=torch.uint8, device=f"cuda:{self.device}")
        else:
            out = np.empty((n, BLOCK_RECORD_BYTES), np.uint8)
        if n:
            self._wait_torch(out)
            _lib.check(fn(*args, _ptr(out), n, _ptr(counts), TSDF_MEM_DEVICE if device else TSDF_MEM_HOST),
                       fn.__name__)
            self._signal_torch(out)
        return counts, out

    def render_bands(self, K, width, height, cam_T_world: SE3, max_depth: float, rows, device=False):
        """(counts per band, records grouped by band) of this shard's blocks the rays of rows
        [rows[b], rows[b + 1]) can read (tsdf_render_bands)."""
        Kc = K._c() if isinstance(K, CameraIntrinsics) else _lib.Intrinsics(*[float(v) for v in K])
        r = np.ascontiguousarray(rows, dtype=np.int32)
        self._rows_keep = r
        L = _lib.load()
        return self._grouped(L.tsdf_render_bands, (self._h, C.byref(Kc), width, height, C.byref(cam_T_world._c()),
                                                   max_depth, r.shape[0] - 1, _ptr(r)), r.shape[0] - 1, device)

    def pack_halo(self, device=False):
        """(counts per destination shard, records grouped by destination) of this shard's blocks that
        other shards' marching cubes read (tsdf_pack_halo)."""
        return self._grouped(_lib.load().tsdf_pack_halo, (self._h,), self.shard_count, device)

    def render_blocks(self, K, width, height, cam_T_world: SE3, max_depth: float, device=False):
        """Records (n, TSDF_BLOCK_RECORD_BYTES) uint8 of the blocks a raycast of this camera can read
        (tsdf_render_blocks): a numpy array, or a torch tensor on this engine's GPU when device."""
        L = _lib.load()
        Kc = K._c() if isinstance(K, CameraIntrinsics) else _lib.Intrinsics(*[float(v) for v in K])
        pc = cam_T_world._c()
        n = C.c_int64()
        _lib.check(L.tsdf_render_blocks(self._h, C.byref(Kc), width, height, C.byref(pc), max_depth,
                                        None, 0, C.byref(n), TSDF_MEM_HOST), "tsdf_render_blocks")
        if device:
            import torch
            out = torch.empty((n.value, BLOCK_RECORD_BYTES), dtype=torch.uint8,
                              device=f"cuda:{self.device}")
            kind = TSDF_MEM_DEVICE
        else:
            out = np.empty((n.value, BLOCK_RECORD_BYTES), np.uint8)
            kind = TSDF_MEM_HOST
        if n.value:
            self._wait_torch(out)
            _lib.check(L.tsdf_render_blocks(self._h, C.byref(Kc), width, height, C.byref(pc),
                                            max_depth, _ptr(out), n.value, C.byref(n), kind),
                       "tsdf_render_blocks")
            self._signal_torch(out)
        return out

    def pack_blocks(self, bounds=None, device=False):
        """Records (n, TSDF_BLOCK_RECORD_BYTES) of the Query block selection (tsdf_pack_blocks;
        bounds None = every live block): numpy, or a torch tensor on this engine's GPU."""
        L = _lib.load()
        b = None if bounds is None else np.ascontiguousarray(
            bounds.as_array() if isinstance(bounds, BoundingCube) else bounds, dtype=np.float32)
        n = C.c_int64()
        _lib.check(L.tsdf_pack_blocks(self._h, _ptr(b), None, 0, C.byref(n), TSDF_MEM_HOST),
                   "tsdf_pack_blocks")
        if device:
            import torch
            out = torch.empty((n.value, BLOCK_RECORD_BYTES), dtype=torch.uint8,
                              device=f"cuda:{self.device}")
        else:
            out = np.empty((n.value, BLOCK_RECORD_BYTES), np.uint8)
        if n.value:
            self._wait_torch(out)
            _lib.check(L.tsdf_pack_blocks(self._h, _ptr(b), _ptr(out), n.value, C.byref(n),
                                          TSDF_MEM_DEVICE if device else TSDF_MEM_HOST),
                       "tsdf_pack_blocks")
            self._signal_torch(out)
        return out

    def import_blocks(self, records, replace=False):
        """Allocate and fill the blocks of render records (tsdf_import_blocks); numpy or GPU tensor.
        replace: empty the volume first, so it holds exactly these blocks."""
        n = int(records.shape[0]) if records.ndim == 2 else int(records.size) // BLOCK_RECORD_BYTES
        kind = TSDF_MEM_DEVICE if _is_torch_cuda(records) else TSDF_MEM_HOST
        if kind == TSDF_MEM_HOST:
            records = np.ascontiguousarray(records, dtype=np.uint8)
        self._wait_torch(records)  # e.g. an all-gather / torch.cat still queued on torch's stream
        _lib.check(_lib.load().tsdf_import_blocks(self._h, _ptr(records), n, kind, int(replace)),
                   "tsdf_import_blocks")
        self._signal_torch(records)

    def reset(self):
        """Empty the volume (tsdf_reset)."""
        _lib.check(_lib.load().tsdf_reset(self._h), "tsdf_reset")

    def extract_mesh(self, bounds=None, missing_tsdf: float = 0.99, min_weight: int = 0,
                     out=None, owner=None) -> np.ndarray:
        """Marching-cubes triangles (n, 3, 3) float32 of the selected blocks (tsdf_extract_mesh).
        out: optional device tensor of >= 9 n floats to receive them on the GPU instead.
        owner: (shard_index, shard_count) -- only the blocks of that shard emit
        (tsdf_extract_mesh_owned; the others are read as neighbours)."""
        L = _lib.load()
        b = None if bounds is None else np.ascontiguousarray(
            bounds.as_array() if isinstance(bounds, BoundingCube) else bounds, dtype=np.float32)
        oi, oc = owner if owner is not None else (0, 1)
        fn = lambda ptr, cap, n, kind: L.tsdf_extract_mesh_owned(self._h, _ptr(b), missing_tsdf, min_weight,
                                                                 oi, oc, ptr, cap, C.byref(n), kind)
        n = C.c_int64()
        if out is not None:  # one call: count, scan and emission enqueued together, one host read
            if not (_is_torch_cuda(out) and out.is_contiguous() and str(out.dtype) == "torch.float32"):
                raise ValueError("out must be a contiguous float32 device tensor")
            self._wait_torch(out)
            _lib.check(fn(_ptr(out), out.numel() // 9, n, TSDF_MEM_DEVICE), "tsdf_extract_mesh")
            self._signal_torch(out)
            return out[:9 * n.value].view(-1, 3, 3)
        _lib.check(fn(None, 0, n, TSDF_MEM_HOST), "tsdf_extract_mesh")
        tris = np.zeros((n.value, 3, 3), np.float32)
        if n.value:
            _lib.check(fn(_ptr(tris), n.value, n, TSDF_MEM_HOST), "tsdf_extract_mesh")
        return tris

    def extract_mesh_indexed(self, bounds=None, missing_tsdf: float = 0.99, min_weight: int = 0,
                             device: bool = False) -> dict:
        """The mesh of extract_mesh with shared vertices and the volume's semantics
        (tsdf_extract_mesh_indexed): a dict of positions (n, 3) f32, rgba (n, 4) u8 (r, g, b, weight),
        prob (n,) f32 (high-touch probability), keys (n, 4) i32 (the vertex's grid edge: global voxel
        coordinate of its lower endpoint, axis) and indices (m, 3) i32; triangle i is triangle i of
        extract_mesh. numpy arrays, or with device=True torch tensors on this engine's GPU written by
        one call (ordered against torch's stream like extract_mesh(out=...))."""
        L = _lib.load()
        b = None if bounds is None else np.ascontiguousarray(
            bounds.as_array() if isinstance(bounds, BoundingCube) else bounds, dtype=np.float32)
        nv, nt = C.c_int64(), C.c_int64()

        def call(m):
            return L.tsdf_extract_mesh_indexed(self._h, _ptr(b), missing_tsdf, min_weight,
                                               None if m is None else C.byref(m), C.byref(nv), C.byref(nt))

        def struct(a, vcap, tcap, kind):
            return _lib.MeshOut(_ptr(a["positions"]), _ptr(a["rgba"]), _ptr(a["prob"]), _ptr(a["keys"]),
                                _ptr(a["indices"]), vcap, tcap, kind)

        if device:
            import torch
            dev = f"cuda:{self.device}"
            vcap, tcap = self._mesh_caps
            for attempt in range(2):  # once more with the returned counts when the guess was too small
                a = dict(positions=torch.empty((vcap, 3), dtype=torch.float32, device=dev),
                         rgba=torch.empty((vcap, 4), dtype=torch.uint8, device=dev),
                         prob=torch.empty((vcap,), dtype=torch.float32, device=dev),
                         keys=torch.empty((vcap, 4), dtype=torch.int32, device=dev),
                         indices=torch.empty((tcap, 3), dtype=torch.int32, device=dev))
                self._wait_torch(*a.values())
                rc = call(struct(a, vcap, tcap, TSDF_MEM_DEVICE))
                self._signal_torch(*a.values())
                if rc != _lib.TSDF_ERR_CAPACITY or attempt == 1:
                    break
                vcap, tcap = nv.value, nt.value
            _lib.check(rc, "tsdf_extract_mesh_indexed")
            # the next call's first guess: this mesh and a quarter
            self._mesh_caps = (nv.value + nv.value // 4 + 1024, nt.value + nt.value // 4 + 1024)
            n, m = nv.value, nt.value
            return {k: (v[:m] if k == "indices" else v[:n]) for k, v in a.items()}
        _lib.check(call(None), "tsdf_extract_mesh_indexed")
        n, m = nv.value, nt.value
        a = dict(positions=np.zeros((n, 3), np.float32), rgba=np.zeros((n, 4), np.uint8),
                 prob=np.zeros(n, np.float32), keys=np.zeros((n, 4), np.int32),
                 indices=np.zeros((m, 3), np.int32))
        if n or m:
            _lib.check(call(struct(a, n, m, TSDF_MEM_HOST)), "tsdf_extract_mesh_indexed")
        return a

    # ---- pose tracking ----
    @staticmethod
    def _Kc(K):
        return K._c() if isinstance(K, CameraIntrinsics) else _lib.Intrinsics(*[float(v) for v in K])

    def raycast_surface(self, K, width, height, cam_T_world: SE3, max_depth: float, device: bool = False,
                        maps=("point", "normal", "depth", "prob", "rgbw")) -> dict:
        """What raycast() sees as float maps (tsdf_raycast_surface): point and normal (h, w, 3) f32 in
        the world frame, depth (h, w) f32 (0 = no surface), prob (h, w) f32 and rgbw (h, w, 4) u8 of
        the hit voxel; a pixel without a surface holds zeros. numpy arrays, or with device=True torch
        tensors on this engine's GPU. `maps` selects the optional ones (point and normal always)."""
        shapes = dict(point=(height, width, 3), normal=(height, width, 3), depth=(height, width),
                      prob=(height, width), rgbw=(height, width, 4))
        names = [k for k in shapes if k in ("point", "normal") or k in maps]
        if device:
            import torch
            a = {k: torch.empty(shapes[k], dtype=torch.uint8 if k == "rgbw" else torch.float32,
                                device=f"cuda:{self.device}") for k in names}
        else:
            a = {k: np.zeros(shapes[k], np.uint8 if k == "rgbw" else np.float32) for k in names}
        out = _lib.SurfaceOut(*(_ptr(a.get(k)) for k in shapes), TSDF_MEM_DEVICE if device else TSDF_MEM_HOST)
        self._wait_torch(*a.values())
        _lib.check(_lib.load().tsdf_raycast_surface(self._h, C.byref(self._Kc(K)), width, height,
                                                    C.byref(cam_T_world._c()), max_depth, C.byref(out)),
                   "tsdf_raycast_surface")
        self._signal_torch(*a.values())
        return a

    def icp_linearize(self, depth, K, cam_T_world: SE3, model: dict, model_K, model_cam_T_world: SE3,
                      stride: int, max_dist: float, max_depth: float):
        """One point-to-plane linearisation (tsdf_icp_linearize) of the depth frame (h, w) f32 at the
        estimate cam_T_world against the point / normal maps of raycast_surface(model_K, ...,
        model_cam_T_world): (A (6, 6), b (6,), sum r^2, count) in float64. depth and the maps are all
        numpy arrays or all torch tensors on this engine's GPU."""
        dev = _is_torch_cuda(depth)
        pt, nr = model["point"], model["normal"]
        if dev != _is_torch_cuda(pt) or dev != _is_torch_cuda(nr):
            raise ValueError("depth and the model maps must be all host or all device")
        if dev:
            import torch
            for a in (depth, pt, nr):
                if a.dtype != torch.float32 or a.device.index != self.device:
                    raise ValueError("device depth and maps must be float32 tensors on this engine's GPU")
            d, pt, nr = depth.contiguous(), pt.contiguous(), nr.contiguous()
        else:
            d, pt, nr = _np(depth, np.float32), _np(pt, np.float32), _np(nr, np.float32)
        h, w = d.shape
        mh, mw = pt.shape[:2]
        m = _lib.IcpModel(_ptr(pt), _ptr(nr), mw, mh, self._Kc(model_K), model_cam_T_world._c())
        out = np.zeros(29, np.float64)
        self._wait_torch(d, pt, nr)
        _lib.check(_lib.load().tsdf_icp_linearize(self._h, _ptr(d), w, h, C.byref(self._Kc(K)),
                                                  C.byref(cam_T_world._c()), C.byref(m), stride, max_dist,
                                                  max_depth, _ptr(out), TSDF_MEM_DEVICE if dev else TSDF_MEM_HOST),
                   "tsdf_icp_linearize")
        self._signal_torch(d, pt, nr)
        A = np.zeros((6, 6), np.float64)
        A[np.triu_indices(6)] = out[:21]
        A = A + np.triu(A, 1).T
        return A, out[21:27].copy(), float(out[27]), int(out[28])

    def point_map_normals(self, model: dict, K, cam_T_world: SE3):
        """The model normals track() uses (tsdf_point_map_normals), from the point / normal maps (h, w, 3)
        f32 of raycast_surface(K, w, h, cam_T_world, ...): the cross product of the points' central
        differences, turned to face the camera, over its length; zeros on the border, beside a hole and
        more than acos(0.3) off the viewing ray. model["normal"] says only where a surface is. Returns
        (h, w, 3) f32: a numpy array for numpy maps, a torch tensor on this engine's GPU for device maps."""
        pt, nr = model["point"], model["normal"]
        dev = _is_torch_cuda(pt)
        if dev != _is_torch_cuda(nr):
            raise ValueError("the model maps must be all host or all device")
        if dev:
            import torch
            for a in (pt, nr):
                if a.dtype != torch.float32 or a.device.index != self.device:
                    raise ValueError("device maps must be float32 tensors on this engine's GPU")
            pt, nr = pt.contiguous(), nr.contiguous()
            out = torch.empty_like(pt)
        else:
            pt, nr = _np(pt, np.float32), _np(nr, np.float32)
            out = np.zeros(pt.shape, np.float32)
        if pt.ndim != 3 or pt.shape[2] != 3 or tuple(nr.shape) != tuple(pt.shape):
            raise ValueError("point and normal must both be (h, w, 3)")
        h, w = pt.shape[:2]
        self._wait_torch(pt, nr, out)
        _lib.check(_lib.load().tsdf_point_map_normals(self._h, C.byref(self._Kc(K)), w, h, C.byref(cam_T_world._c()),
                                                      _ptr(pt), _ptr(nr), _ptr(out),
                                                      TSDF_MEM_DEVICE if dev else TSDF_MEM_HOST),
                   "tsdf_point_map_normals")
        self._signal_torch(pt, nr, out)
        return out

    def track(self, depth, K, guess: SE3, max_depth: float, **cfg):
        """The pose of a depth frame (h, w) f32 against the volume (tsdf_track): frame-to-model
        point-to-plane ICP from `guess`. Keywords are tsdf_track_config's fields (levels, stride,
        iterations, max_dist, eps_rot, eps_trans, min_inliers). Returns (SE3 cam_T_world, info) with
        info = dict(status, iterations, inliers, rmse); status 1 (degenerate) keeps the last good estimate."""
        L = _lib.load()
        c = _lib.TrackConfig()
        L.tsdf_track_config_default(C.byref(c))
        for k, v in cfg.items():
            if k in ("stride", "iterations"):
                v = list(v) + [1] * (3 - len(v))
                setattr(c, k, (C.c_int * 3)(*[int(x) for x in v]))
            elif k in ("levels", "min_inliers"):
                setattr(c, k, int(v))
            elif k in ("max_dist", "eps_rot", "eps_trans"):
                setattr(c, k, float(v))
            else:
                raise TypeError(f"track: unknown option {k}")
        dev = _is_torch_cuda(depth)
        d = depth.contiguous() if dev else _np(depth, np.float32)
        h, w = d.shape
        r = _lib.TrackResult()
        self._wait_torch(d)
        _lib.check(L.tsdf_track(self._h, _ptr(d), w, h, TSDF_MEM_DEVICE if dev else TSDF_MEM_HOST,
                                C.byref(self._Kc(K)), C.byref(guess._c()), max_depth, C.byref(c), C.byref(r)),
                   "tsdf_track")
        self._signal_torch(d)
        p = r.cam_T_world
        return (SE3((p.qx, p.qy, p.qz, p.qw), (p.tx, p.ty, p.tz)),
                dict(status=int(r.status), iterations=int(r.iterations), inliers=int(r.inliers), rmse=float(r.rmse)))

    # ---- what the array calls below share (surface_normals .. view_gain) ----
    @staticmethod
    def _kind(device):
        return TSDF_MEM_DEVICE if device else TSDF_MEM_HOST

    def _alloc(self, shape, dtype, device, zero=False):
        """An empty (zero=True: zeroed) array of a numpy dtype: numpy for a host call, a torch tensor on this
        engine's GPU for a device call."""
        if device:
            import torch
            return (torch.zeros if zero else torch.empty)(shape, dtype=getattr(torch, np.dtype(dtype).name),
                                                          device=f"cuda:{self.device}")
        return (np.zeros if zero else np.empty)(shape, dtype)

    @staticmethod
    def _box(origin, dims, who=""):
        """(o, d, shape) of a box: origin (None: a call that takes dims alone) and dims as lists of three ints,
        and the shape (nz, ny, nx) of its arrays. `who` opens the error text."""
        d = [int(v) for v in dims]
        o = None if origin is None else [int(v) for v in origin]
        if len(d) != 3 or (o is not None and len(o) != 3):
            raise ValueError(who + ("dims are three integers" if o is None else
                                    "origin and dims are three integers each"))
        return o, d, (d[2], d[1], d[0])

    @staticmethod
    def _box_ok(d):
        """The library's box limits (TSDF_BOX_MAX_DIM, TSDF_BOX_MAX_VOXELS)."""
        return all(1 <= v <= _lib.TSDF_BOX_MAX_DIM for v in d) and d[0] * d[1] * d[2] <= _lib.TSDF_BOX_MAX_VOXELS

    @staticmethod
    def _same_box(a, o, d):
        """Whether the dict `a` (a travel field, a layer) lies over the box o, d."""
        return [int(v) for v in a["dims"]] == list(d) and [int(v) for v in a["origin"]] == list(o)

    def _call(self, name, tensors, fn, *args, allow=()):
        """fn(handle, *args) between the two orderings with torch's stream for `tensors` (None entries are
        skipped): wait, call, signal, then check -- a failed call has signalled before it raises. Returns the
        code, which is TSDF_OK or one of `allow`."""
        self._wait_torch(*tensors)
        rc = fn(self._h, *args)
        self._signal_torch(*tensors)
        if rc not in allow:
            _lib.check(rc, name)
        return rc

    # ---- UV dose ----
    def _points(self, a, device, cols=3):
        """An (n, cols) f32 array as the call takes it (cols=1: (n,); cols=None: any 2-D matrix): a
        contiguous numpy array, or with device=True a contiguous torch tensor on this engine's GPU."""
        if device:
            import torch
            t = a if _is_torch_cuda(a) else torch.as_tensor(np.asarray(a, np.float32), device=f"cuda:{self.device}")
            t = t.to(torch.float32).contiguous()
        else:
            if _is_torch_cuda(a):
                raise ValueError("device tensors need device=True")
            t = np.ascontiguousarray(a, dtype=np.float32)
        if cols is None:
            if t.ndim != 2:
                raise ValueError(f"expected a 2-D matrix, got {tuple(t.shape)}")
            return t
        if (cols == 1 and t.ndim != 1) or (cols > 1 and (t.ndim != 2 or t.shape[1] != cols)):
            raise ValueError(f"expected shape (n{', %d' % cols if cols > 1 else ''}), got {tuple(t.shape)}")
        return t

    def surface_normals(self, points, sample_offset: float = 0.0, device: bool = False):
        """The unit normal of the voxel nearest to each of the (n, 3) world points (tsdf_surface_normals):
        its six-neighbour central difference over its length, zeros where that is zero or not finite.
        sample_offset 0.5 for mesh vertices (the mesh's half-voxel shift), 0 for raycast_surface points.
        numpy in and out, or with device=True torch tensors on this engine's GPU."""
        p = self._points(points, device)
        out = self._alloc(tuple(p.shape), np.float32, device, zero=not device)
        self._call("tsdf_surface_normals", (p, out), _lib.load().tsdf_surface_normals, _ptr(p), p.shape[0],
                   float(sample_offset), _ptr(out), self._kind(device))
        return out

    def uv_dose(self, points, normals, emitters, dose=None, device: bool = False, **cfg):
        """The UV dose [J/m^2] the point emitters add to each receiver (tsdf_uv_dose): inverse-square and
        cosine law, an emitter counting only where a shadow ray through the volume reaches it. points,
        normals (n, 3) f32 (normals=None: surface_normals(points, sample_offset)); emitters (m, 4) f32
        rows x, y, z, energy [J] on the host (uv.tube_emitters); dose (n,) f32 to accumulate into (None:
        zeros; a given array or tensor of the right kind is updated in place). Keywords are
        tsdf_uv_config's fields (bias, step, min_range, max_range, sample_offset, min_weight, use_grid).
        Returns the dose array, or with device=True the tensor."""
        c, p, nr, em = self._uv_inputs("uv_dose", points, normals, emitters, device, cfg)
        n = p.shape[0]
        d = self._alloc((n,), np.float32, device, zero=True) if dose is None else self._points(dose, device, cols=1)
        if tuple(nr.shape) != tuple(p.shape) or d.shape[0] != n:
            raise ValueError("points, normals and dose do not match")
        self._call("tsdf_uv_dose", (p, nr, d), _lib.load().tsdf_uv_dose, _ptr(p), _ptr(nr), n, _ptr(em), em.shape[0],
                   C.byref(c), _ptr(d), self._kind(device))
        return d

    def _uv_inputs(self, what, points, normals, emitters, device, cfg):
        """What uv_dose and uv_irradiance share: (tsdf_uv_config from the keywords, points, normals -- the
        surface's own when None -- and the emitters as (m, 4) f32 on the host)."""
        c = _lib.UvConfig()
        _lib.load().tsdf_uv_config_default(self._h, C.byref(c))
        for k, v in cfg.items():
            if k in ("min_weight", "use_grid"):
                setattr(c, k, int(v))
            elif k in ("bias", "step", "min_range", "max_range", "sample_offset"):
                setattr(c, k, float(v))
            else:
                raise TypeError(f"{what}: unknown option {k}")
        p = self._points(points, device)
        nr = self.surface_normals(p, c.sample_offset, device) if normals is None else self._points(normals, device)
        return c, p, nr, np.ascontiguousarray(emitters, dtype=np.float32).reshape(-1, 4)

    # ---- lamp-stop planning ----
    def uv_irradiance(self, points, normals, emitters, first, device: bool = False, **cfg):
        """The dose [J/m^2] each of C candidate lamp placements alone would add to each receiver
        (tsdf_uv_irradiance): row c is what uv_dose writes into zeros given only emitters[first[c]:first[c + 1]],
        bit for bit, from one call. points, normals (n, 3) f32 (normals=None: surface_normals); emitters
        (m, 4) f32 and first (C + 1,) int32 on the host (uv.tube_candidates), first[0] == 0, non-decreasing,
        first[-1] == m. Keywords are tsdf_uv_config's fields, as uv_dose's. Returns (C, n) f32: a numpy
        array, or with device=True a tensor on this engine's GPU."""
        c, p, nr, em = self._uv_inputs("uv_irradiance", points, normals, emitters, device, cfg)
        fi = np.ascontiguousarray(first, dtype=np.int32).reshape(-1)
        if tuple(nr.shape) != tuple(p.shape):
            raise ValueError("points and normals do not match")
        if fi.size < 1 or int(fi[-1]) != em.shape[0]:
            raise _lib.TSDFError("tsdf_uv_irradiance: invalid argument (first holds C + 1 offsets and ends at the "
                                 "number of emitters)")
        n, nc = p.shape[0], fi.size - 1
        out = self._alloc((nc, n), np.float32, device)
        self._call("tsdf_uv_irradiance", (p, nr, out), _lib.load().tsdf_uv_irradiance, _ptr(p), _ptr(nr), n, _ptr(em),
                   _ptr(fi), nc, C.byref(c), _ptr(out), self._kind(device))
        return out

    def uv_plan(self, irradiance, need, weight=None, max_stops: int = 16, min_gain: float = 0.0,
                device: bool = False):
        """Greedy lamp stops on a (C, n) irradiance matrix (tsdf_uv_plan): each round picks the candidate that
        removes the most weighted missing dose, sum over i of weight[i] * min(E[c][i], need[i]) (the lowest
        index between equal gains), and subtracts its row from need, until max_stops rounds ran or the best
        gain is not positive or below min_gain. need (n,) f32 [J/m^2] (uv.plan_need), weight (n,) f32 or None
        for all 1 (uv.vertex_area * prob). Deterministic: the same inputs give the same bits. Returns
        dict(stops (k,) int32, gains (k,) f64, need (n,) f32: what is still missing after the stops); need is
        a new array, or with device=True a new tensor (irradiance and need may be tensors then)."""
        E = self._points(irradiance, device, cols=None)
        nc, n = int(E.shape[0]), int(E.shape[1])
        if device:
            nd = self._points(need, device, cols=1).clone()
        else:
            nd = np.array(need, dtype=np.float32, order="C", copy=True)
            if nd.ndim != 1:
                raise ValueError("need: expected shape (n,)")
        w = None if weight is None else self._points(weight, device, cols=1)
        if nd.shape[0] != n or (w is not None and w.shape[0] != n):
            raise ValueError("irradiance, need and weight do not match")
        c = _lib.UvPlanConfig(int(max_stops), float(min_gain))
        k = max(int(max_stops), 0)
        stops, gains, num = np.zeros(k, np.int32), np.zeros(k, np.float64), C.c_int32(0)
        self._call("tsdf_uv_plan", (E, nd, w), _lib.load().tsdf_uv_plan, _ptr(E), nc, n, _ptr(nd), _ptr(w), C.byref(c),
                   _ptr(stops), _ptr(gains), C.byref(num), self._kind(device))
        return dict(stops=stops[:num.value].copy(), gains=gains[:num.value].copy(), need=nd)

    # ---- distance field ----
    def distance_field(self, origin, dims, max_dist: int = 255, min_weight: int = 1, unknown: bool = False,
                       state: bool = True, device: bool = False):
        """The exact squared Euclidean distance [voxels^2], saturated at max_dist^2, from every voxel of a
        box to the nearest surface voxel inside the box (tsdf_distance_field). origin: the box's first
        voxel (global voxel coordinates x, y, z), dims: (nx, ny, nz). A surface voxel is observed (its
        block exists, weight >= min_weight), has tsdf <= 0 and a free face neighbour; with unknown=True
        every unobserved voxel of the box is a site as well. Only sites inside the box count: pad a region
        by max_dist. Returns dict(d2 (nz, ny, nx) uint16, state (same shape uint8: 0 unobserved, 1 free,
        2 inside; None with state=False), origin, dims, max_dist, unknown): numpy arrays, or with
        device=True torch tensors on this engine's GPU, ordered after the call on torch's current stream.
        esdf.metres / esdf.signed / esdf.clearance turn the field into metres."""
        L = _lib.load()
        c = _lib.EdtConfig()
        L.tsdf_edt_config_default(C.byref(c))
        o, d, shape = self._box(origin, dims)
        c.origin, c.dims = (C.c_int32 * 3)(*o), (C.c_int32 * 3)(*d)
        c.max_dist, c.min_weight = int(max_dist), int(min_weight)
        c.sites = _lib.TSDF_EDT_SURFACE | (_lib.TSDF_EDT_UNKNOWN if unknown else 0)
        if not self._box_ok(d):  # (a refused box allocates nothing: one element stands in for the outputs)
            shape = (1,)
        d2 = self._alloc(shape, np.uint16, device)
        st = self._alloc(shape, np.uint8, device) if state else None
        out = _lib.EdtOut(_ptr(d2), _ptr(st), self._kind(device))
        self._call("tsdf_distance_field", (d2, st), L.tsdf_distance_field, C.byref(c), C.byref(out))
        return dict(d2=d2, state=st, origin=tuple(o), dims=tuple(d), max_dist=int(max_dist), unknown=bool(unknown))

    # ---- travel field ----
    def _box_array(self, a, dtype, shape, device, what):
        """A field array of the box as a call takes it: contiguous numpy, or with device=True a contiguous
        tensor on this engine's GPU (a host array is uploaded)."""
        if device:
            import torch
            tdt = {np.uint16: torch.uint16, np.uint8: torch.uint8, np.uint32: torch.uint32}[dtype]
            t = a if _is_torch_cuda(a) else torch.as_tensor(np.ascontiguousarray(a, dtype=dtype),
                                                            device=f"cuda:{self.device}")
            if t.dtype != tdt:
                raise ValueError(f"{what}: expected dtype {tdt}")
            t = t.contiguous()
        else:
            if _is_torch_cuda(a):
                t = a.cpu().numpy()
            else:
                t = a
            t = np.ascontiguousarray(t, dtype=dtype)
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{what}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
        return t

    def travel_field(self, field, seeds, clearance2: int = 0, unknown_free: bool = False, device: bool = False):
        """The least travel cost from the seed voxels to every voxel of a distance field's box through
        passable voxels (tsdf_travel_field). field: a distance_field result that has state. A voxel is
        passable when d2 >= clearance2 and its state is 1 (observed free) or, with unknown_free, 0
        (unobserved: the optimistic planner -- an unobserved gap in a wall leaks). Steps go to the 26
        neighbours and cost 3 / 4 / 5 (face / edge / corner), so cost / 3 is a length in voxels;
        clearance2 >= 4 keeps a diagonal step from slipping between two surface voxels that touch at a
        corner. seeds: (S, 3) global voxel coordinates (esdf.voxel_of); seeds outside the box or impassable
        are ignored. Returns dict(cost (nz, ny, nx) uint32: 0 at the seeds, 0xFFFFFFFF where unreached,
        origin, dims, seeded: seeds used, rounds: relaxation rounds run): numpy, or with device=True a torch
        tensor on this engine's GPU, ordered after the call on torch's current stream. Does not touch the
        volume: pending frames stay pending, and a shard engine serves as well."""
        L = _lib.load()
        if field.get("state") is None:
            raise ValueError("travel_field: the field has no state (distance_field(..., state=True))")
        o, d, shape = self._box(field["origin"], field["dims"], "travel_field: ")
        d2 = self._box_array(field["d2"], np.uint16, shape, device, "d2")
        st = self._box_array(field["state"], np.uint8, shape, device, "state")
        s = np.ascontiguousarray(np.asarray(seeds, np.int64).reshape(-1, 3) - np.asarray(o, np.int64))
        s = np.ascontiguousarray(np.clip(s, -(1 << 30), 1 << 30).astype(np.int32))
        c = _lib.TravelConfig()
        L.tsdf_travel_config_default(C.byref(c))
        c.dims = (C.c_int32 * 3)(*d)
        c.clearance2, c.unknown_free = int(clearance2), 1 if unknown_free else 0
        cost = self._alloc(shape, np.uint32, device)
        seeded, rounds = C.c_int32(0), C.c_int32(0)
        self._call("tsdf_travel_field", (d2, st, cost), L.tsdf_travel_field, C.byref(c), _ptr(d2), _ptr(st),
                   _ptr(s) if s.shape[0] else None, int(s.shape[0]), _ptr(cost), self._kind(device), C.byref(seeded),
                   C.byref(rounds))
        return dict(cost=cost, origin=tuple(o), dims=tuple(d), seeded=seeded.value, rounds=rounds.value)

    def travel_paths(self, travel, targets, max_len: int = 4096):
        """The path from each target back to a seed over a travel_field result (tsdf_travel_paths): a list
        of int32 arrays of box-local linear voxel indices (z * ny + y) * nx + x, the target first and the
        seed last (esdf.path_points turns them into world positions). targets: (T, 3) global voxel
        coordinates. An unreached target or one outside the box gives an empty array. Asks again with a
        longer max_len when a path was truncated. A field this library did not write may have no
        predecessor somewhere: ValueError."""
        L = _lib.load()
        _, d, shape = self._box(None, travel["dims"], "travel_paths: ")
        cost = travel["cost"]
        device = _is_torch_cuda(cost)
        if not device:
            cost = np.ascontiguousarray(cost, dtype=np.uint32)
        elif not cost.is_contiguous():
            cost = cost.contiguous()
        if tuple(cost.shape) != shape:
            raise ValueError("travel_paths: cost does not match dims")
        t = np.asarray(targets, np.int64).reshape(-1, 3) - np.asarray(travel["origin"], np.int64)
        t = np.ascontiguousarray(np.clip(t, -(1 << 30), 1 << 30).astype(np.int32))
        nt = int(t.shape[0])
        if nt == 0:
            return []
        dims = (C.c_int32 * 3)(*d)
        max_len = min(max(int(max_len), 1), 1 << 28)
        out, k0 = [], 0
        while k0 < nt:
            n = min(nt - k0, max((1 << 28) // max_len, 1))  # (a call takes T * max_len <= 2^28)
            tk = np.ascontiguousarray(t[k0:k0 + n])
            path, ln = np.zeros((n, max_len), np.int32), np.zeros(n, np.int32)
            self._call("tsdf_travel_paths", (cost,), L.tsdf_travel_paths, dims, _ptr(cost), self._kind(device), _ptr(tk),
                       n, max_len, _ptr(path), _ptr(ln))
            if (ln < 0).any():
                raise ValueError("travel_paths: the field has a voxel without a predecessor (not a travel_field result)")
            if int(ln.max()) > max_len:  # (a path visits a voxel once: at most 2^28, one target per call then)
                max_len = int(ln.max())
                continue
            out += [path[k, :ln[k]].copy() for k in range(n)]
            k0 += n
        return out

    # ---- observed free space ----
    def _free_box(self, layer):
        """(tsdf_free_box, the layer's words as the calls take them, whether they are device memory)."""
        o, d, _ = self._box(layer["origin"], layer["dims"], "a layer's ")
        bits = layer["bits"]
        device = _is_torch_cuda(bits)
        if device:
            import torch
            if bits.dtype != torch.int32 or not bits.is_contiguous():
                raise ValueError("a device layer's bits are a contiguous torch.int32 tensor")
            n = bits.numel()
        else:
            if not (isinstance(bits, np.ndarray) and bits.dtype == np.uint32 and bits.flags.c_contiguous):
                raise ValueError("a host layer's bits are a contiguous numpy uint32 array")
            n = bits.size
        if n != max(d[2], 0) * max(d[1], 0) * ((max(d[0], 0) + 31) // 32):
            raise ValueError("the layer's bits do not match its dims: nz * ny * ceil(nx / 32) words")
        return _lib.FreeBox((C.c_int32 * 3)(*o), (C.c_int32 * 3)(*d)), bits, device

    def free_observe(self, layer, depth, K, cam_T_world: SE3, max_depth: float):
        """Marks in `layer` (esdf.free_layer) every voxel of its box that this depth frame saw as free
        (tsdf_free_observe): the voxel update's own projection, with sdf >= truncation and the voxel in front
        of the camera plane, whether or not the voxel's block exists. bits |= free: idempotent and monotone.
        depth: (H, W) float32, a host array or a device tensor; it is moved to where the layer's bits are.
        A device layer's call is asynchronous on the engine stream. Does not touch the volume: pending
        frames stay pending, and a shard engine serves as well. Returns the layer."""
        L = _lib.load()
        box, bits, device = self._free_box(layer)
        if device:
            import torch
            dp = depth if _is_torch_cuda(depth) else torch.as_tensor(np.ascontiguousarray(depth, dtype=np.float32),
                                                                     device=bits.device)
            if dp.dtype != torch.float32:
                raise ValueError("free_observe: depth must be float32")
            dp = dp.contiguous()
        else:
            dp = np.ascontiguousarray(depth.cpu().numpy() if _is_torch_cuda(depth) else depth, dtype=np.float32)
        if dp.ndim != 2:
            raise ValueError("free_observe: depth is (H, W)")
        h, w = int(dp.shape[0]), int(dp.shape[1])
        self._call("tsdf_free_observe", (bits, dp), L.tsdf_free_observe, C.byref(box), _ptr(bits), _ptr(dp), w, h,
                   self._kind(device), C.byref(self._Kc(K)), C.byref(cam_T_world._c()), float(max_depth))
        return layer

    def free_apply(self, layer, field, count: bool = True):
        """A distance field with its state promoted from 0 (unobserved) to 1 (free) wherever the layer's
        bit is set (tsdf_free_apply); states 1 and 2 and voxels outside the layer's box stay. Returns a new
        field dict: `state` a promoted copy where the layer's bits are (numpy for a host layer, a tensor
        for a device layer), `promoted` the number of voxels changed (None with count=False, which keeps a
        device call asynchronous), everything else -- d2 included -- shared with `field`. Hand it to
        travel_field(..., unknown_free=False)."""
        L = _lib.load()
        box, bits, device = self._free_box(layer)
        if field.get("state") is None:
            raise ValueError("free_apply: the field has no state (distance_field(..., state=True))")
        o, d, shape = self._box(field["origin"], field["dims"], "free_apply: ")
        st = self._box_array(field["state"], np.uint8, shape, device, "state")
        st = st.clone() if device else st.copy()
        n = C.c_int64(0)
        self._call("tsdf_free_apply", (bits, st), L.tsdf_free_apply, C.byref(box), _ptr(bits), (C.c_int32 * 3)(*o),
                   (C.c_int32 * 3)(*d), _ptr(st), self._kind(device), C.byref(n) if count else None)
        return dict(field, state=st, promoted=int(n.value) if count else None)

    # ---- frontiers and components ----
    def frontier_mask(self, field, travel=None, device: bool = False, count: bool = True):
        """The frontier of a distance field (tsdf_frontier_mark): mask 1 at every observed-free voxel
        (state 1) that has an unobserved (state 0) face neighbour inside the box and, with `travel` (a
        travel_field result over the same box), that the travel field reached. field should have been
        promoted by free_apply and built from surface sites only (unknown=False). Returns dict(mask
        (nz, ny, nx) uint8, marked: the number of ones (None with count=False, which keeps a device call
        asynchronous), origin, dims): numpy, or with device=True a torch tensor on this engine's GPU. Does
        not touch the volume: pending frames stay pending, and a shard engine serves as well."""
        L = _lib.load()
        if field.get("state") is None:
            raise ValueError("frontier_mask: the field has no state (distance_field(..., state=True))")
        o, d, shape = self._box(field["origin"], field["dims"], "frontier_mask: ")
        if travel is not None and not self._same_box(travel, o, d):
            raise ValueError("frontier_mask: the travel field's box is not the distance field's")
        st = self._box_array(field["state"], np.uint8, shape, device, "state")
        cost = None if travel is None else self._box_array(travel["cost"], np.uint32, shape, device, "cost")
        mask = self._alloc(shape, np.uint8, device)
        n = C.c_int64(0)
        self._call("tsdf_frontier_mark", (st, cost, mask), L.tsdf_frontier_mark, (C.c_int32 * 3)(*d), _ptr(st),
                   _ptr(cost), _ptr(mask), self._kind(device), C.byref(n) if count else None)
        return dict(mask=mask, marked=int(n.value) if count else None, origin=tuple(o), dims=tuple(d))

    def components(self, mask, dims, key=None, min_size: int = 1, device: bool = False):
        """The 26-connected components of a voxel mask over a box (tsdf_components). mask: (nz, ny, nx)
        uint8, members nonzero; dims: (nx, ny, nz); key: optional uint32 array of the same shape (a travel
        field's cost). Returns dict(label (nz, ny, nx) uint32: the least linear index (z * ny + y) * nx + x
        among the members of the voxel's component, 0xFFFFFFFF off the mask; clusters: a numpy structured
        array (COMPONENT_DTYPE: label, size, lo, hi, sum, goal, goal_key) of the components with size >=
        min_size in ascending label -- goal the member with the least key, ties to the least index, label
        without key; count = len(clusters); total: all components). label is numpy, or with device=True a
        torch tensor on this engine's GPU. Does not touch the volume."""
        L = _lib.load()
        _, d, shape = self._box(None, dims)
        if not self._box_ok(d):  # (a refused box: the arrays keep the mask's shape and the library says why)
            shape = tuple(np.shape(mask))
        m = self._box_array(mask, np.uint8, shape, device, "mask")
        k = None if key is None else self._box_array(key, np.uint32, shape, device, "key")
        label = self._alloc(shape, np.uint32, device)
        c = _lib.ComponentsConfig()
        L.tsdf_components_config_default(C.byref(c))
        c.dims, c.min_size = (C.c_int32 * 3)(*d), int(min_size)
        count, total = C.c_int32(0), C.c_int32(0)
        # the two-call pattern with a first guess: a table too small asks again with the count it was told
        cap = 4096
        for retry in ((_lib.TSDF_ERR_CAPACITY,), ()):
            clusters = np.zeros(cap, COMPONENT_DTYPE)
            rc = self._call("tsdf_components", (m, k, label), L.tsdf_components, C.byref(c), _ptr(m), _ptr(k),
                            _ptr(label), self._kind(device), _ptr(clusters), cap, C.byref(count), C.byref(total),
                            allow=retry)
            if rc != _lib.TSDF_ERR_CAPACITY:
                break
            cap = int(count.value)
        return dict(label=label, clusters=clusters[:count.value].copy(), count=int(count.value),
                    total=int(total.value))

    def frontiers(self, field, travel=None, min_size: int = 1, device: bool = False):
        """Where the map ends, as clusters (frontier_mask, then components with key = travel["cost"]):
        dict(mask, marked, label, clusters, count, total, origin, dims). A cluster's goal is then its
        cheapest voxel to travel to and goal_key that cost (esdf.frontier_goals gives world positions and
        metres, esdf.frontier_voxels a cluster's voxels)."""
        fm = self.frontier_mask(field, travel, device=device)
        cc = self.components(fm["mask"], fm["dims"], key=None if travel is None else travel["cost"],
                             min_size=min_size, device=device)
        return dict(fm, **cc)

    # ---- view gain ----
    def view_gain(self, field_or_state, views, K, width: int, height: int, far: float, step=None, margin=None,
                  miss_depth=None, seen=None, depth: bool = False, device: bool = False):
        """The unobserved voxels each candidate camera pose would observe (tsdf_view_gain). field_or_state:
        a distance_field / free_apply result (dict with state, origin, dims) or a tuple (state, origin, dims),
        state (nz, ny, nx) uint8; views: a list of SE3 (cam_T_world); K: the views' intrinsics. Each view's
        depth image is predicted by marching its rays `far` metres in steps of `step` (default: the voxel
        size) to the first state-2 voxel -- miss_depth (default far; 0: no return) where there is none --
        and gain[i] counts the state-0 voxels, outside the layer `seen` (esdf.free_layer over the same box)
        when given, that free_observe would mark from that image with truncation `margin` (default: the
        engine's). Returns dict(gain (V,) int64, depth (V, H, W) float32 or None, origin, dims): numpy, or
        with device=True the depth a torch tensor on this engine's GPU (state and seen are uploaded when
        they are host arrays). Does not touch the volume: pending frames stay pending, and a shard engine
        serves as well."""
        L = _lib.load()
        if isinstance(field_or_state, dict):
            if field_or_state.get("state") is None:
                raise ValueError("view_gain: the field has no state (distance_field(..., state=True))")
            state, origin, dims = field_or_state["state"], field_or_state["origin"], field_or_state["dims"]
        else:
            state, origin, dims = field_or_state
        o, d, shape = self._box(origin, dims, "view_gain: ")
        st = self._box_array(state, np.uint8, shape, device, "state")
        bits = None
        if seen is not None:
            if not self._same_box(seen, o, d):
                raise ValueError("view_gain: the seen layer's box is not the state's")
            bits = seen["bits"]
            wshape = (d[2], d[1], (d[0] + 31) // 32)
            if device:
                import torch
                if not _is_torch_cuda(bits):
                    bits = torch.as_tensor(np.ascontiguousarray(bits, dtype=np.uint32).view(np.int32),
                                           device=f"cuda:{self.device}")
                if bits.dtype != torch.int32:
                    raise ValueError("view_gain: a device layer's bits are torch.int32")
                bits = bits.contiguous()
            else:
                bits = bits.cpu().numpy().view(np.uint32) if _is_torch_cuda(bits) else bits
                bits = np.ascontiguousarray(bits, dtype=np.uint32)
            if tuple(bits.shape) != wshape:
                raise ValueError(f"view_gain: seen bits: expected shape {wshape}, got {tuple(bits.shape)}")
        views = list(views)
        nv, w, h = len(views), int(width), int(height)
        c = _lib.ViewConfig()
        L.tsdf_view_config_default(self._h, C.byref(c))
        c.origin, c.dims = (C.c_int32 * 3)(*o), (C.c_int32 * 3)(*d)
        c.width, c.height = w, h
        c.K = self._Kc(K)
        c.far = float(far)
        c.miss_depth = float(far) if miss_depth is None else float(miss_depth)
        if step is not None:
            c.step = float(step)
        if margin is not None:
            c.margin = float(margin)
        poses = (_lib.Pose * max(nv, 1))(*[v._c() for v in views])
        gain = np.zeros(nv, np.int64)
        out = self._alloc((nv, max(h, 0), max(w, 0)), np.float32, device) if depth else None
        self._call("tsdf_view_gain", (st, bits, out), L.tsdf_view_gain, C.byref(c), _ptr(st), _ptr(bits),
                   C.cast(poses, C.c_void_p), nv, _ptr(gain), _ptr(out) if nv else None, self._kind(device))
        return dict(gain=gain, depth=out, origin=tuple(o), dims=tuple(d))

    def query(self, bounds=None) -> np.ndarray:
        L = _lib.load()
        b = None if bounds is None else np.ascontiguousarray(
            bounds.as_array() if isinstance(bounds, BoundingCube) else bounds, dtype=np.float32)
        n = C.c_int64()
        _lib.check(L.tsdf_query(self._h, _ptr(b), None, 0, C.byref(n)), "tsdf_query")
        out = np.zeros(n.value, VOXEL_DTYPE)
        if n.value:
            _lib.check(L.tsdf_query(self._h, _ptr(b), out.ctypes.data_as(C.c_void_p), n.value,
                                    C.byref(n)), "tsdf_query")
        return out

    def snapshot(self) -> np.ndarray:
        """The whole volume between frames as bytes (tsdf_snapshot_save): restore() on an engine
        of the same voxel size, truncation and pool size continues the stream bit for bit."""
        L = _lib.load()
        n = C.c_int64()
        _lib.check(L.tsdf_snapshot_bytes(self._h, C.byref(n)), "tsdf_snapshot_bytes")
        buf = np.empty(n.value, np.uint8)
        _lib.check(L.tsdf_snapshot_save(self._h, _ptr(buf), n.value), "tsdf_snapshot_save")
        return buf

    def restore(self, snapshot):
        buf = np.ascontiguousarray(snapshot, dtype=np.uint8)
        _lib.check(_lib.load().tsdf_snapshot_load(self._h, _ptr(buf), buf.size), "tsdf_snapshot_load")

    def stats(self, clear_status=False) -> dict:
        s = _lib.Stats()
        _lib.check(_lib.load().tsdf_get_stats(self._h, C.byref(s), int(clear_status)), "tsdf_get_stats")
        return {k: getattr(s, k) for k, _ in _lib.Stats._fields_}

    def profile_begin(self, integrate_only: bool = False, every: int = 1, kernel_events: bool = False):
        """HIP-event timing of every `every`-th following integrate call: all phases (marker
        events between them), only k_integrate (marker events around it), or -- kernel_events --
        k_integrate's own dispatch timestamps (start/stop events bound to the launch)."""
        mode = 2 if kernel_events else (1 if integrate_only else 0)
        _lib.check(_lib.load().tsdf_profile_begin(self._h, mode, every), "tsdf_profile_begin")

    def profile_end(self) -> dict:
        p = _lib.Profile()
        _lib.check(_lib.load().tsdf_profile_end(self._h, C.byref(p)), "tsdf_profile_end")
        return {k: getattr(p, k) for k, _ in _lib.Profile._fields_}

    def dump(self, pool: bool = True) -> dict:
        pos = np.zeros((NUM_ENTRY, 4), np.int16)
        idx = np.zeros(NUM_ENTRY, np.int32)
        heap = np.zeros(self.num_blocks, np.int32)
        free = np.zeros(1, np.int32)
        out = dict(entry_pos=pos, entry_idx=idx, heap=heap)
        tsdf = prob = rgbw = None
        if pool:
            nv = self.num_blocks * BLOCK_VOLUME
            tsdf = np.zeros(nv, np.float32)
            prob = np.zeros(nv, np.float32)
            rgbw = np.zeros((nv, 4), np.uint8)
            out.update(tsdf=tsdf, prob=prob, rgbw=rgbw)
        _lib.check(_lib.load().tsdf_debug_dump(self._h, _ptr(pos), _ptr(idx), _ptr(heap), _ptr(free),
                                               _ptr(tsdf), _ptr(prob), _ptr(rgbw)), "tsdf_debug_dump")
        out["free"] = int(free[0])
        return out

    # ---- VoxelHashTable / VoxelMemPool level ----
    def hash_allocate(self, keys):
        k = np.ascontiguousarray(keys, dtype=np.int16).reshape(-1, 3)
        _lib.check(_lib.load().tsdf_hash_allocate(self._h, _ptr(k), k.shape[0]), "tsdf_hash_allocate")

    def hash_delete(self, keys):
        k = np.ascontiguousarray(keys, dtype=np.int16).reshape(-1, 3)
        _lib.check(_lib.load().tsdf_hash_delete(self._h, _ptr(k), k.shape[0]), "tsdf_hash_delete")

    def hash_retrieve(self, points) -> dict:
        p = np.ascontiguousarray(points, dtype=np.int16).reshape(-1, 3)
        n = p.shape[0]
        rgbw = np.zeros((n, 4), np.uint8)
        tsdf = np.zeros(n, np.float32)
        prob = np.zeros(n, np.float32)
        bpo = np.zeros((n, 4), np.int16)
        bidx = np.zeros(n, np.int32)
        _lib.check(_lib.load().tsdf_hash_retrieve(self._h, _ptr(p), n, _ptr(rgbw), _ptr(tsdf),
                                                  _ptr(prob), _ptr(bpo), _ptr(bidx)), "tsdf_hash_retrieve")
        return dict(rgbw=rgbw, tsdf=tsdf, prob=prob, block_pos_off=bpo, block_idx=bidx)

    def hash_assign(self, points, rgbw) -> int:
        p = np.ascontiguousarray(points, dtype=np.int16).reshape(-1, 3)
        v = np.ascontiguousarray(rgbw, dtype=np.uint8).reshape(-1, 4)
        missing = C.c_int()
        _lib.check(_lib.load().tsdf_hash_assign(self._h, _ptr(p), p.shape[0], _ptr(v),
                                                C.byref(missing)), "tsdf_hash_assign")
        return missing.value

    def num_active_blocks(self) -> int:
        n = C.c_int32()
        _lib.check(_lib.load().tsdf_num_active_blocks(self._h, C.byref(n)), "tsdf_num_active_blocks")
        return n.value

    def pool_acquire(self, n: int) -> np.ndarray:
        out = np.zeros(n, np.int32)
        _lib.check(_lib.load().tsdf_pool_acquire(self._h, n, _ptr(out)), "tsdf_pool_acquire")
        return out

    def pool_release(self, idx):
        i = np.ascontiguousarray(idx, dtype=np.int32)
        _lib.check(_lib.load().tsdf_pool_release(self._h, _ptr(i), i.shape[0]), "tsdf_pool_release")

    def pool_set_weight(self, block: int, w: int):
        _lib.check(_lib.load().tsdf_pool_set_weight(self._h, int(block), int(w)), "tsdf_pool_set_weight")

    def pool_get_weights(self, block: int) -> np.ndarray:
        out = np.zeros(BLOCK_VOLUME, np.uint8)
        _lib.check(_lib.load().tsdf_pool_get_weights(self._h, int(block), _ptr(out)), "tsdf_pool_get_weights")
        return out


def _engine_call(fn):
    """Every public Engine method that enters the library settles a pending deferred raycast after
    its call (Engine._after_call)."""
    def wrapper(self, *a, **k):
        prev = self._pending
        r = fn(self, *a, **k)
        self._after_call(prev)
        return r
    wrapper.__name__, wrapper.__doc__, wrapper.__wrapped__ = fn.__name__, fn.__doc__, fn
    return wrapper


for _name, _fn in list(vars(Engine).items()):
    if callable(_fn) and not _name.startswith("_") and _name not in ("close", "frame_graph", "shard_frame_graph") \
            and not isinstance(_fn, (staticmethod, classmethod)):
        setattr(Engine, _name, _engine_call(_fn))
del _name, _fn


class Group:
    """One volume spatially sharded over `devices` (one shard per entry; a device may repeat) with the
    exchange inside the library (tsdf_group_*, csrc/tsdf_group.hip): each shard's update kernel
    writes its carve candidates into every shard's inbox, so a frame is one launch per shard and no
    collective. Same results as one volume (the union of the shards)."""

    def __init__(self, devices, voxel_size=0.005, truncation=0.03, max_width=1920, max_height=1080,
                 num_block_bits=18):
        L = _lib.load()
        cfg = _lib.Config()
        L.tsdf_config_default(C.byref(cfg))
        cfg.voxel_size, cfg.truncation = voxel_size, truncation
        cfg.max_width, cfg.max_height, cfg.num_block_bits = max_width, max_height, num_block_bits
        devs = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        _lib.check(L.tsdf_group_create(C.byref(cfg), devs, len(devices), C.byref(h)), "tsdf_group_create")
        self._g = h
        self.n = len(devices)
        self.devices = list(devices)
        self.num_blocks = 1 << num_block_bits
        self.voxel_size, self.truncation = voxel_size, truncation

    def integrate(self, rgb, depth, ht, lt, K, cam_T_world: SE3, max_depth: float):
        """Host arrays, or device tensors on devices[0] (contiguous; torch's stream is synchronised
        first: the group runs on its own streams, and torch's current stream is ordered after the
        group's work afterwards -- tsdf_group_stream_signal -- so the frame's tensors may be reused or
        freed on it)."""
        dev = _is_torch_cuda(depth)
        if dev:
            import torch
            torch.cuda.current_stream().synchronize()
            for a in (rgb, depth, ht, lt):
                if a is not None and not a.is_contiguous():
                    raise ValueError("device frames must be contiguous")
            H, W = int(depth.shape[0]), int(depth.shape[1])
        else:
            rgb, depth = _np(rgb, np.uint8), _np(depth, np.float32)
            ht, lt = _np(ht, np.float32), _np(lt, np.float32)
            H, W = depth.shape
        fr = _lib.Frame(W, H, _ptr(rgb), _ptr(depth), _ptr(ht), _ptr(lt), TSDF_MEM_DEVICE if dev else TSDF_MEM_HOST)
        Kc = K._c() if isinstance(K, CameraIntrinsics) else _lib.Intrinsics(*[float(v) for v in K])
        L = _lib.load()
        _lib.check(L.tsdf_group_integrate(self._g, C.byref(fr), C.byref(Kc), C.byref(cam_T_world._c()), max_depth),
                   "tsdf_group_integrate")
        if dev:
            _lib.check(L.tsdf_group_stream_signal(self._g, C.c_void_p(_current_raw_stream(self.devices[0]))),
                       "tsdf_group_stream_signal")

    def flush(self):
        _lib.check(_lib.load().tsdf_group_flush(self._g), "tsdf_group_flush")

    def synchronize(self):
        _lib.check(_lib.load().tsdf_group_synchronize(self._g), "tsdf_group_synchronize")

    def stats(self, clear_status=False) -> dict:
        s = _lib.Stats()
        _lib.check(_lib.load().tsdf_group_get_stats(self._g, C.byref(s), int(clear_status)), "tsdf_group_get_stats")
        return {k: getattr(s, k) for k, _ in _lib.Stats._fields_}

    def query(self, bounds=None) -> np.ndarray:
        b = None if bounds is None else np.ascontiguousarray(
            bounds.as_array() if isinstance(bounds, BoundingCube) else bounds, dtype=np.float32)
        n = C.c_int64()
        L = _lib.load()
        _lib.check(L.tsdf_group_query(self._g, _ptr(b), None, 0, C.byref(n)), "tsdf_group_query")
        out = np.zeros(n.value, VOXEL_DTYPE)
        if n.value:
            _lib.check(L.tsdf_group_query(self._g, _ptr(b), out.ctypes.data_as(C.c_void_p), n.value, C.byref(n)),
                       "tsdf_group_query")
        return out

    def raycast(self, K, width, height, cam_T_world: SE3, max_depth: float):
        Kc = K._c() if isinstance(K, CameraIntrinsics) else _lib.Intrinsics(*[float(v) for v in K])
        rgba = np.zeros((height, width, 4), np.uint8)
        normal = np.zeros((height, width, 4), np.uint8)
        _lib.check(_lib.load().tsdf_group_raycast(self._g, C.byref(Kc), width, height, C.byref(cam_T_world._c()),
                                                  max_depth, _ptr(rgba), _ptr(normal), TSDF_MEM_HOST),
                   "tsdf_group_raycast")
        return rgba, normal

    def shard(self, i: int) -> "Engine":
        """Shard i's engine (tsdf_group_shard: completes the pending frames first), a borrowed handle
        the group owns -- for dumps, statistics and profiling of one shard; do not close it."""
        h = C.c_void_p()
        _lib.check(_lib.load().tsdf_group_shard(self._g, i, C.byref(h)), "tsdf_group_shard")
        eng = Engine.__new__(Engine)
        eng._h, eng.num_blocks, eng._pending, eng._stream = h, self.num_blocks, None, -1
        eng.device, eng.shard_index, eng.shard_count = self.devices[i], i, self.n
        eng.voxel_size, eng.truncation = self.voxel_size, self.truncation
        eng.close = lambda: None  # (borrowed)
        return eng

    def shard_dump(self, i: int, pool: bool = True) -> dict:
        """tsdf_debug_dump of shard i's engine (tsdf_group_shard)."""
        return self.shard(i).dump(pool)

    def close(self):
        if getattr(self, "_g", None):
            _lib.load().tsdf_group_destroy(self._g)
            self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ShardGroup:
    """G shard engines of one spatially sharded volume on ONE GPU, exchanging their key
    and carve-candidate slots with device copies where a multi-GPU job all-gathers them
    (tsdf_amd.dist.integrate_sharded). The engines run on torch's current stream, so the copies are
    ordered between the phases. For tests and single-GPU rehearsals of the sharded path.
    split: True -- shard i runs the DDA over tile-row band i of G and the keys are exchanged;
    False -- every shard runs the whole frame's DDA, only carve candidates are exchanged."""

    def __init__(self, shard_count: int, voxel_size=0.005, truncation=0.03, max_width=1920,
                 max_height=1080, num_block_bits=18, device=0, key_cap=16384, cand_cap=16384,
                 split=True, stream=None, graph=None, pipe=False):
        import torch
        self.G = shard_count
        # pipe: pipelined sharded frames (tsdf_integrate_shard_pipe, one exchange per frame, every shard
        # runs the whole DDA); reads of the volume need flush() first
        self.pipe = pipe
        if pipe and (split or graph is not None):
            raise ValueError("pipelined sharded frames run the whole DDA on every shard (split=False, no graph)")
        self.graph_size = graph  # (width, height): frames through each shard's captured graph
        self.split = split
        self.key_cap, self.cand_cap = key_cap, cand_cap
        # all shards on ONE stream (torch's current one unless given), so the phases and the slot
        # reads / writes between them are ordered
        stream = torch.cuda.current_stream(device) if stream is None else stream
        self.engines = [Engine(voxel_size, truncation, max_width, max_height, num_block_bits, device,
                               shard_index=i, shard_count=shard_count, stream=stream)
                        for i in range(shard_count)]
        dev = f"cuda:{device}"
        self._keys = torch.zeros((shard_count, Engine.shard_slot_bytes(key_cap)), dtype=torch.uint8, device=dev)
        self._cands = torch.zeros((shard_count, Engine.shard_slot_bytes(cand_cap)), dtype=torch.uint8, device=dev)
        self.keys_exchanged = 0   # key records that went through the exchange (all frames)
        self.cands_exchanged = 0  # carve-candidate records likewise
        self.cands_by_shard = [0] * shard_count  # ... by the shard that sent them
        # pipelined: call n writes its candidates into slot set n % 2 and reads set (n - 1) % 2 (the
        # "all-gather" of the previous call: every shard's slot)
        self._pc = torch.zeros((2, shard_count, Engine.shard_slot_bytes(cand_cap)), dtype=torch.uint8,
                               device=dev) if pipe else None
        self._ncall = 0
        self.graphs = None
        if graph is not None:
            w, h = graph
            self.graphs = [e.shard_frame_graph(w, h, i if split else 0, shard_count if split else 1)
                           for i, e in enumerate(self.engines)]

    def integrate(self, rgb, depth, ht, lt, K, cam_T_world: SE3, max_depth: float, count=False):
        try:
            self._integrate(rgb, depth, ht, lt, K, cam_T_world, max_depth, count)
        except Exception:
            self._abort_all()
            raise

    def _abort_all(self):
        # no shard stays stuck mid-frame (three-call frames and pipelined ones alike); every shard is
        # aborted even if one abort fails, and the caller sees the original error
        for e in self.engines:
            try:
                e.integrate_shard_abort()
            except Exception:
                pass

    def _pipe_step(self, rgb, depth, ht, lt, K, cam_T_world, max_depth):
        out, inb = self._pc[self._ncall & 1], self._pc[(self._ncall + 1) & 1]
        # (the call counter moves even when a shard fails part-way: the aborted shards restart from
        # "no pending frame", whose first call reads no inbox)
        self._ncall += 1
        pend = [e.integrate_shard_pipe(rgb, depth, ht, lt, K, cam_T_world, max_depth, inb, out[i], self.cand_cap)
                for i, e in enumerate(self.engines)]
        return any(pend)

    def flush(self):
        """Pipelined: complete the pending frames (steps with their exchanges); a no-op otherwise."""
        if self.pipe:
            try:
                while self._pipe_step(None, None, None, None, None, None, 4.0):
                    pass
            except Exception:
                self._abort_all()
                raise

    def _integrate(self, rgb, depth, ht, lt, K, cam_T_world, max_depth, count):
        G = self.G
        if self.pipe:
            self._pipe_step(rgb, depth, ht, lt, K, cam_T_world, max_depth)
            # this call's slots hold the candidates of the frame it updated
            self._count(count, cands=self._pc[(self._ncall - 1) & 1])
            return
        if self.graphs is not None:
            for i, g in enumerate(self.graphs):
                g.begin(rgb, depth, ht, lt, K, cam_T_world, max_depth, self._keys[i], self._keys, self.key_cap,
                        self._cands[i], self._cands, self.cand_cap)
            for g in self.graphs:
                g.update()
            for g in self.graphs:
                g.end()
            self._count(count)
            return
        for i, e in enumerate(self.engines):
            if self.split:
                e.integrate_shard_begin(rgb, depth, ht, lt, K, cam_T_world, max_depth, i, G, self._keys[i],
                                        self.key_cap)
            else:
                e.integrate_shard_begin(rgb, depth, ht, lt, K, cam_T_world, max_depth)
        keys_in = self._keys if self.split else None  # the all-gathered key slots
        for i, e in enumerate(self.engines):
            e.integrate_shard_update(keys_in, self.key_cap, self._cands[i], self.cand_cap)
        for e in self.engines:
            e.integrate_shard_end(self._cands, self.cand_cap)
        self._count(count)

    def _count(self, count, cands=None):
        if not count:
            return
        import torch
        cands = self._cands if cands is None else cands
        # per-shard candidate counts (slot headers: record 0's count word), a host sync
        per = cands[:, 8:12].contiguous().view(torch.int32).view(-1).tolist()
        self.cands_by_shard = [a + b for a, b in zip(self.cands_by_shard, per)]
        if self.split:
            self.keys_exchanged += int(self._keys[:, 8:12].contiguous().view(torch.int32).sum())
        self.cands_exchanged += sum(per)

    def synchronize(self):
        self.flush()
        for e in self.engines:
            e.synchronize()

    def stats(self):
        self.flush()
        return [e.stats() for e in self.engines]

    def close(self):
        for g in self.graphs or []:
            g.close()
        for e in self.engines:
            e.close()


class TSDFGrid:
    """voxel_tsdf.cuh:32-124 TSDFGrid(voxel_size, truncation) on the MI355X engine."""

    def __init__(self, voxel_size: float, truncation: float, **engine_kw):
        self.engine = Engine(voxel_size=voxel_size, truncation=truncation, **engine_kw)

    def Integrate(self, img_rgb, img_depth, img_ht, img_lt, max_depth: float,
                  intrinsics: CameraIntrinsics, cam_T_world: SE3):
        """voxel_tsdf.cu:347-375. img_ht / img_lt are required here as in the reference."""
        self.engine.integrate(img_rgb, img_depth, img_ht, img_lt, intrinsics, cam_T_world, max_depth)

    def RayCast(self, max_depth: float, virtual_cam: CameraParams, cam_T_world: SE3):
        """voxel_tsdf.cu:490-506; returns (rgba, normal) HxWx4 uint8 images."""
        return self.engine.raycast(virtual_cam.intrinsics, virtual_cam.img_w, virtual_cam.img_h,
                                   cam_T_world, max_depth)

    def GatherValid(self) -> np.ndarray:
        """voxel_tsdf.cu:399-425."""
        return self.engine.query(None)

    def GatherVoxels(self, volumn: BoundingCube) -> np.ndarray:
        """voxel_tsdf.cu:427-454."""
        return self.engine.query(volumn)

    def close(self):
        self.engine.close()
