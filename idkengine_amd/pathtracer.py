"""PathTracer — host-side mirror of IDKEngine's `class PathTracer` (Source/Render/PathTracer.cs:10-365) over the
C-ABI of libidkpt.so.  Same property names, same reset-accumulation behaviour, same lifecycle
(ctor(width,height,settings) / Compute() / SetSize / ResetAccumulation / Dispose); the implicit GL bindings the
reference's shaders read become the explicit UploadScene / SetCamera calls.  The C# drop-in that binds the same
entry points through LibraryImport is shown in INTEGRATION.md.

No CPU fallback: construction raises when libidkpt.so or a GPU is missing.
"""
import ctypes as C
import os
import numpy as np
from . import _lib
from . import gputypes as T
from ._lib import IdkPtError


# idkptSetDeveloperOption names; IDKPT_<NAME> in the environment is forwarded when a PathTracer is created (test / tuning hooks only)
_OPTION_NAMES = ("force_generic", "no_tile_cull", "no_lean_primary", "leaf_min", "grab_unit_log2", "grab_fixed", "lds_pad", "trace_waves", "grid_hint", "grid_rays_x4", "grid_mid_waves", "defer_last", "last_occlusion", "fold_last", "split", "split_donor", "split_peek", "group_threads", "query_scheduler", "split_scatter", "fused", "fused_shade_min", "leaf_pool", "pool_min", "adv_min",
                 "wide", "wide_cap", "wide_count", "packet", "packet_min_live", "packet_waves", "inst_tlas", "inst_tlas_overlap", "inst_braid", "inst_unify", "inst_unify_radius", "uni_refill", "inst_general", "pair_nodes", "inst_sieve", "inst_sieve_overlap", "gen_pixel_major", "gen_group_max", "bounce_pixel_major", "transport", "bvh_timing", "bvh_small", "bvh_stackopt_host", "force_no_peer", "download_member", "trace_variant")


class PathTracer:
    def __init__(self, width, height, settings=None, device=0, row_modulo=1, row_remainder=0, devices=None, row_band=1):
        """devices: list of HIP device ids for ONE context that renders on several GPUs (idkptCreate(deviceCount = N)); an id may repeat
        (two members on one GPU).  Otherwise one device (`device`), optionally one row shard of a process-per-GPU run (row_modulo/remainder;
        row_band: rows are dealt in bands of that many rows, idkptSetRowBands)."""
        self._L = _lib.load()
        n = C.c_int32(0)
        self._L.idkptGetDeviceCount(C.byref(n))
        if n.value <= 0:
            raise IdkPtError("no HIP device visible: the path tracer has no CPU fallback")
        ctx = C.c_void_p()
        ids = list(devices) if devices else [device]
        self.device_count = len(ids); self.device_ids = ids
        if self.device_count > 1 and (row_modulo, row_remainder) != (1, 0):
            raise IdkPtError("a multi-device context deals its rows itself")
        dev = (C.c_int32 * len(ids))(*ids)
        rc = self._L.idkptCreate(len(ids), dev, C.byref(ctx))
        if rc != 0:
            raise IdkPtError(f"idkptCreate failed with status {rc}")
        self._ctx = ctx
        # tuning / test options: the library reads no environment; this host mirror forwards IDKPT_<NAME> (tests, tools) to idkptSetDeveloperOption
        for name in _OPTION_NAMES:
            v = os.environ.get("IDKPT_" + name.upper())
            if v is not None and v != "":
                self.set_option(name, int(v))
        self._settings = settings if settings is not None else T.Settings.default()
        self._cached_ray_depth = self._settings.RayDepth
        self._scene = None
        self.width, self.height = width, height
        self.row_modulo, self.row_remainder, self.row_band = row_modulo, row_remainder, (int(row_band) if row_modulo > 1 else 1)
        self._row_limit = None
        if self.device_count == 1:
            if self.row_band > 1:
                self._check(self._L.idkptSetRowBands(ctx, self.row_band, row_modulo, row_remainder))
            else:
                self._check(self._L.idkptSetRowSharding(ctx, row_modulo, row_remainder))
        self._check(self._L.idkptSetSize(ctx, width, height))
        self._push_settings()

    # ------------------------------------------------------------------ plumbing
    def _check(self, rc):
        err = getattr(self, "_callback_error", None)
        if err is not None:            # an exchange callback raised while the library was inside a launch (ctypes cannot propagate it): re-raise here
            self._callback_error = None
            raise err
        if rc != 0:
            msg = C.c_char_p()
            self._L.idkptGetLastError(self._ctx, C.byref(msg))
            raise IdkPtError(f"idkpt status {rc}: {(msg.value or b'').decode()}")

    def _push_settings(self):
        self._check(self._L.idkptSetSettings(self._ctx, C.addressof(self._settings)))

    def global_rows(self):
        """image rows of this context's local rows, in local order"""
        b = self.row_band
        ys = [y for y in range(self.height) if (y // b) % self.row_modulo == self.row_remainder] if self.row_modulo > 1 else list(range(self.row_remainder, self.height))
        return ys if self._row_limit is None else ys[:self._row_limit]

    @property
    def rows(self):
        return len(self.global_rows())

    # ------------------------------------------------------------------ PathTracer.cs public surface
    def _prop(name, gpu=False):  # noqa: N805
        def get(self):
            return getattr(self._settings.Gpu if gpu else self._settings, name)

        def set_(self, v):
            setattr(self._settings.Gpu if gpu else self._settings, name, type(get(self))(v))
            self._push_settings()
        return property(get, set_)

    SamplesPerPixel = _prop("SamplesPerPixel")        # PathTracer.cs:12
    RayDepth = _prop("RayDepth")                      # :16-25 (resets accumulation)
    FocalLength = _prop("FocalLength", gpu=True)      # :39-48
    LenseRadius = _prop("LenseRadius", gpu=True)      # :50-59
    DoTraceLights = _prop("DoTraceLights", gpu=True)  # :83-92
    DoRussianRoulette = _prop("DoRussianRoulette", gpu=True)  # :94-102
    DoRaySorting = _prop("DoRaySorting")              # :104-114
    OutputAOVs = _prop("OutputAOVs")                  # :116-125
    UseTlas = _prop("UseTlas")                        # BVH.GpuUseTlas (Bvh/BVH.cs:16-26)
    BlasStackSize = _prop("BlasStackSize")            # BVH.BlasStackSize (Bvh/BVH.cs:28-45)

    @property
    def DoDebugBVHTraversal(self):                    # :61-81
        return self._settings.Gpu.DoDebugBVHTraversal == 1

    @DoDebugBVHTraversal.setter
    def DoDebugBVHTraversal(self, value):
        self._settings.Gpu.DoDebugBVHTraversal = 1 if value else 0
        if value:
            self._cached_ray_depth = self._settings.RayDepth
            self._settings.RayDepth = 1
        else:
            self._settings.RayDepth = self._cached_ray_depth
        self._push_settings()
        self.ResetAccumulation()

    @property
    def AccumulatedSamples(self):                     # :27-37
        v = C.c_uint32()
        self._check(self._L.idkptGetAccumulatedSamples(self._ctx, C.byref(v)))
        return v.value

    def Compute(self):                                # :214-271
        self._check(self._L.idkptRender(self._ctx))

    def SetSize(self, width, height):                 # :299-332
        self.width, self.height = width, height
        self._check(self._L.idkptSetSize(self._ctx, width, height))

    def SetPresentationSize(self, width, height):     # Application.SetResolutions(renderRes, presentRes), Application.cs:570-586
        """idkptSetPresentationSize: the size of the display image (Present) and of bloom's chain and expanded image (Bloom); (0, 0) = the render size, the default.  Kept by
        SetSize; touches neither the images nor the accumulation.  While it differs from the render size Present and Bloom need one device that holds the whole frame."""
        self._check(self._L.idkptSetPresentationSize(self._ctx, int(width), int(height)))

    @property
    def presentation_size(self):
        """idkptGetPresentationSize: the effective (width, height) — the render size while none is set"""
        w, h = C.c_int32(), C.c_int32()
        self._check(self._L.idkptGetPresentationSize(self._ctx, C.byref(w), C.byref(h)))
        return w.value, h.value

    def _display_shape(self):
        """(rows, width) of the display image: the presentation size where it differs from the render size (whole frame), this context's rows otherwise"""
        pw, ph = self.presentation_size
        return (ph, pw) if (pw, ph) != (self.width, self.height) else (self.rows, self.width)

    def SetSampleSequence(self, first, stride):
        """Sample-parallel rendering (idkptSetSampleSequence): this context renders the reference's samples first, first + stride, ..."""
        self._check(self._L.idkptSetSampleSequence(self._ctx, int(first), int(stride)))

    def ResetAccumulation(self):                      # :334-337
        self._check(self._L.idkptResetAccumulation(self._ctx))

    def Dispose(self):                                # :344-365
        if self._ctx:
            self._L.idkptDestroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.Dispose()
        except Exception:
            pass

    @property
    def Result(self):                                 # :143 (Texture.Download equivalent)
        return self.download(0)

    @property
    def AlbedoTexture(self):                          # :167
        return self.download(1)

    @property
    def NormalTexture(self):                          # :168
        return self.download(2)

    # ------------------------------------------------------------------ explicit inputs (implicit GL bindings in the reference)
    def UploadScene(self, scene):
        d, keep = scene.desc()
        self._check(self._L.idkptUploadScene(self._ctx, C.addressof(d)))
        del keep
        self._scene = scene
        if self._settings.BlasStackSize == 0 and scene.blas_stack_size:
            pass  # library derives the LDS stack depth from BlasDescs when BlasStackSize == 0

    def SetCamera(self, cam):
        ip = np.ascontiguousarray(cam.inv_projection, np.float32); iv = np.ascontiguousarray(cam.inv_view, np.float32); vp = np.ascontiguousarray(cam.position, np.float32)
        self._check(self._L.idkptSetPerFrame(self._ctx, ip.ctypes.data, iv.ctypes.data, vp.ctypes.data))

    def SetPerFrameData(self, per_frame):
        """idkptSetPerFrameData: one gputypes.GpuPerFrameData record, taken as it is (the library reads InvProjection, InvView and ViewPos)."""
        p = np.ascontiguousarray(per_frame, T.GpuPerFrameData).reshape(-1)
        if len(p) != 1:
            raise ValueError("SetPerFrameData: one GpuPerFrameData record")
        self._check(self._L.idkptSetPerFrameData(self._ctx, p.ctypes.data))

    def UpdateBuffer(self, which, array, offset_bytes=0):
        a = np.ascontiguousarray(array)
        self._check(self._L.idkptUpdateBuffer(self._ctx, which, offset_bytes, a.nbytes, a.ctypes.data))

    def DownloadBuffer(self, which, dtype, count, offset_bytes=0):
        out = np.zeros(count, dtype)
        self._check(self._L.idkptDownloadBuffer(self._ctx, which, offset_bytes, out.nbytes, out.ctypes.data))
        return out

    def BuildTlas(self, nodes):
        n = np.ascontiguousarray(nodes)
        self._check(self._L.idkptBuildTlas(self._ctx, n.ctypes.data, len(n)))

    def BuildTlasOnDevice(self, search_radius=15):
        """BVH.TlasBuild on the device from the resident BLAS roots / instances / mesh transforms (Bvh/BVH.cs:278-298)."""
        self._check(self._L.idkptBuildTlasOnDevice(self._ctx, search_radius))

    def TraceRays(self, rays, any_hit=False, trace_lights=False):
        """Batched TraceRay / TraceRayAny calls (Shaders/include/BVHIntersect.glsl:183-411) with per-ray maxDist.
        rays: array of gputypes.RayQuery; returns an array of gputypes.RayHit."""
        from . import gputypes as T
        if hasattr(rays, "data_ptr") and getattr(rays, "is_cuda", False):
            # rays already resident on this context's device (a torch tensor of count x 32 bytes, any dtype): the device entry point, no PCIe round trip (2 885 vs 252 Mray/s,
            # profiles/r04_queries.md) — the hits come back as a device tensor (count x 8 float32 words = gputypes.RayHit records), asynchronously in the context's stream order
            import torch
            count = rays.numel() * rays.element_size() // T.RayQuery.itemsize
            hit_bytes = T.RayHit.itemsize
            hits = torch.empty(count * hit_bytes // 4, dtype=torch.float32, device=rays.device)
            self.TraceRaysDevice(rays.data_ptr(), hits.data_ptr(), count, any_hit=any_hit, trace_lights=trace_lights)
            self.synchronize()
            return hits.view(count, hit_bytes // 4)
        r = np.ascontiguousarray(rays, T.RayQuery)
        out = np.zeros(len(r), T.RayHit)
        flags = (T.IDKPT_TRACE_ANY_HIT if any_hit else 0) | (T.IDKPT_TRACE_LIGHTS if trace_lights else 0)
        self._check(self._L.idkptTraceRays(self._ctx, r.ctypes.data, len(r), flags, out.ctypes.data))
        return out

    def TraceShadows(self, params, depth, normal_oct, visibility=None):
        """Shaders/ShadowsRayTraced/compute.glsl for one point shadow.  depth (H,W), normal_oct (H,W,2); returns visibility (H,W)."""
        import ctypes as C
        d = np.ascontiguousarray(depth, np.float32); n = np.ascontiguousarray(normal_oct, np.float32)
        v = np.zeros(d.shape, np.float32) if visibility is None else np.ascontiguousarray(visibility, np.float32).copy()
        self._check(self._L.idkptTraceShadows(self._ctx, C.addressof(params), d.ctypes.data, n.ctypes.data, v.ctypes.data))
        return v

    def TraceRaysDevice(self, d_rays, d_hits, count, any_hit=False, trace_lights=False):
        """idkptTraceRaysDevice: d_rays / d_hits are device pointers (ints, e.g. torch tensor.data_ptr()) on this context's device: count x 32 B each.
        Asynchronous in the context's stream order; synchronize() completes it."""
        from . import gputypes as T
        flags = (T.IDKPT_TRACE_ANY_HIT if any_hit else 0) | (T.IDKPT_TRACE_LIGHTS if trace_lights else 0)
        self._check(self._L.idkptTraceRaysDevice(self._ctx, int(d_rays), int(count), flags, int(d_hits)))

    def TraceShadowsDevice(self, params, d_depth, d_normal_oct, d_visibility):
        """idkptTraceShadowsDevice: the three images are device pointers (W*H floats, W*H*2 floats, W*H floats in/out).  Asynchronous in stream order."""
        import ctypes as C
        self._check(self._L.idkptTraceShadowsDevice(self._ctx, C.addressof(params), int(d_depth), int(d_normal_oct), int(d_visibility)))

    def CollideSpheres(self, spheres, test_steps=1, recursive_steps=8, epsilon=0.001, response=0, use_tlas=False):
        """idkptCollideSpheres: Intersections.SceneVsMovingSphereCollisionRoutine (Source/Shapes/Intersections.cs:491-593) for every sphere, on the resident BVH.
        spheres: array of gputypes.MovingSphere; returns an array of gputypes.SphereCollision.  response: 0 none, 1 slide (the camera), 2 reflect (the lights).
        A contiguous torch tensor on this context's device (count x 48 bytes, any dtype) goes through idkptCollideSpheresDevice instead: no PCIe round trip, the
        results come back as a device tensor of count x 24 float32 words (gputypes.SphereCollision records)."""
        import ctypes as C
        from . import gputypes as T
        st = T.CollideSettings(int(test_steps), int(recursive_steps), float(epsilon), int(response), 1 if use_tlas else 0)
        if hasattr(spheres, "data_ptr"):
            import torch
            if not spheres.is_cuda or spheres.device.index != self.device_ids[0]:
                raise ValueError(f"CollideSpheres: the tensor lives on {spheres.device}, this context on device {self.device_ids[0]}")
            if not spheres.is_contiguous():
                raise ValueError("CollideSpheres: the tensor must be contiguous")
            nbytes = spheres.numel() * spheres.element_size()
            if nbytes % T.MovingSphere.itemsize:
                raise ValueError("CollideSpheres: the tensor is not a whole number of 48-byte gputypes.MovingSphere records")
            count = nbytes // T.MovingSphere.itemsize
            out = torch.empty((count, T.SphereCollision.itemsize // 4), dtype=torch.float32, device=spheres.device)
            self._check(self._L.idkptCollideSpheresDevice(self._ctx, C.addressof(st), spheres.data_ptr() if count else 0, count, out.data_ptr() if count else 0))
            self.synchronize()
            return out
        s = np.ascontiguousarray(spheres, T.MovingSphere).reshape(-1)
        out = np.zeros(len(s), T.SphereCollision)
        self._check(self._L.idkptCollideSpheres(self._ctx, C.addressof(st), s.ctypes.data, len(s), out.ctypes.data))
        return out

    def RefitBlas(self, blas_id):
        self._check(self._L.idkptRefitBlas(self._ctx, blas_id))

    def UploadUnskinnedVertices(self, verts):
        v = np.ascontiguousarray(verts)
        self._check(self._L.idkptUploadUnskinnedVertices(self._ctx, v.ctypes.data, len(v)))

    def Skin(self, input_offset, output_offset, joint_offset, count):
        self._check(self._L.idkptSkin(self._ctx, input_offset, output_offset, joint_offset, count))

    def SetSceneVersions(self, versions):
        """idkptSetSceneVersions: up to `versions` states of the animated geometry in flight (scene updates no longer launch the queued samples first)."""
        self._check(self._L.idkptSetSceneVersions(self._ctx, int(versions)))

    def SetGroupSharding(self, mode):
        """idkptSetGroupSharding: 0 auto (= bands of 8 rows at every RayDepth, with the per-band count exchange beyond 2), 1 rows, 2 strips + device-side count exchange, 3 bands of 8 rows."""
        self._check(self._L.idkptSetGroupSharding(self._ctx, int(mode)))

    def SetRowRange(self, first_row, row_count):
        """idkptSetRowRange: this context renders the contiguous strip [first_row, first_row + row_count)."""
        self._check(self._L.idkptSetRowRange(self._ctx, int(first_row), int(row_count)))
        self.row_modulo, self.row_remainder, self._row_limit, self.row_band = 1, int(first_row), int(row_count), 1

    def SetBounceExchange(self, fn):
        """idkptSetBounceExchange: fn(bounce, local_counts ndarray[samples]) -> bases ndarray[samples] (alive rays of the same sample
        held by the contexts that own earlier rows); None disables.  Needed for exact N-GPU == 1-GPU results beyond RayDepth 2."""
        import ctypes as C
        old = getattr(self, "_xfn", None)   # the library launches what is queued before it swaps the pointer: the old trampoline must outlive the call
        if fn is None:
            self._check(self._L.idkptSetBounceExchange(self._ctx, None, None))
            self._xfn = None; del old
            return
        proto = C.CFUNCTYPE(None, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32))

        def tramp(user, bounce, n, counts, out):
            try:
                b = fn(int(bounce), np.array([counts[i] for i in range(n)], np.uint32))
                for i in range(n):
                    out[i] = int(b[i])
            except BaseException as e:     # ctypes would swallow it and leave `out` unfilled: zero the bases and re-raise from the next _check
                for i in range(n):
                    out[i] = 0
                self._callback_error = e
        new = proto(tramp)
        self._check(self._L.idkptSetBounceExchange(self._ctx, new, None))
        self._xfn = new; del old       # keep the trampoline alive as long as the context uses it

    def SetBandExchange(self, fn):
        """idkptSetBandExchange (interleaved rows / bands): fn(bounce, local_counts ndarray[samples, bands]) -> bases ndarray[samples, bands] = alive rays of the same
        sample, over ALL contexts, in the image bands before each of this context's bands; None disables.  Exact N-GPU == 1-GPU results at any RayDepth (sorting off)."""
        import ctypes as C
        old = getattr(self, "_bxfn", None)   # (see SetBounceExchange: released only after the library has swapped the pointer)
        if fn is None:
            self._check(self._L.idkptSetBandExchange(self._ctx, None, None))
            self._bxfn = None; del old
            return
        proto = C.CFUNCTYPE(None, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32))

        def tramp(user, bounce, samples, bands, counts, out):
            n = samples * bands
            try:
                b = np.asarray(fn(int(bounce), np.ctypeslib.as_array(counts, shape=(n,)).astype(np.uint32).reshape(samples, bands)), np.uint32).reshape(-1)
                for i in range(n):
                    out[i] = int(b[i])
            except BaseException as e:
                for i in range(n):
                    out[i] = 0
                self._callback_error = e
        new = proto(tramp)
        self._check(self._L.idkptSetBandExchange(self._ctx, new, None))
        self._bxfn = new; del old      # keep the trampoline alive as long as the context uses it

    def SetBandExchangeDevice(self, fn):
        """idkptSetBandExchangeDevice: fn(bounce, samples, bands, d_counts_ptr, d_bases_ptr, hip_stream_ptr) ENQUEUES on that stream whatever fills the bases (device
        pointers to uint32[samples * bands]) and returns; no host synchronisation.  None disables."""
        import ctypes as C
        old = getattr(self, "_bxdfn", None)
        if fn is None:
            self._check(self._L.idkptSetBandExchangeDevice(self._ctx, None, None))
            self._bxdfn = None; del old
            return
        proto = C.CFUNCTYPE(None, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p)

        def tramp(user, bounce, samples, bands, d_counts, d_bases, stream):
            try:
                fn(int(bounce), int(samples), int(bands), int(d_counts or 0), int(d_bases or 0), int(stream or 0))
            except BaseException as e:     # (nothing was enqueued: the bases of this bounce are whatever the buffer held; the error surfaces at the next _check)
                self._callback_error = e
        new = proto(tramp)
        self._check(self._L.idkptSetBandExchangeDevice(self._ctx, new, None))
        self._bxdfn = new; del old     # keep the trampoline alive as long as the context uses it

    def transport_info(self):
        """idkptGetTransportInfo: how a multi-device context moves its bulk device-to-device traffic ('none' | 'peer-copy' | 'rccl'), the RCCL ranks, version, and the library path / the reason RCCL is not in use."""
        kind = C.c_int32(); ranks = C.c_int32(); ver = C.c_int32(); detail = C.c_char_p()
        self._check(self._L.idkptGetTransportInfo(self._ctx, C.byref(kind), C.byref(ranks), C.byref(ver), C.byref(detail)))
        return {"transport": ("none", "peer-copy", "rccl")[kind.value], "rccl_ranks": ranks.value, "rccl_version": ver.value, "detail": (detail.value or b"").decode()}

    @staticmethod
    def transport_self_test(device=0):
        """idkptTransportSelfTest: (status, rccl version, detail) of a one-rank RCCL round trip on `device`."""
        L = _lib.load(); ver = C.c_int32(); buf = C.create_string_buffer(512)
        rc = L.idkptTransportSelfTest(device, C.byref(ver), buf, 512)
        return rc, ver.value, buf.value.decode()

    def synchronize(self):
        self._check(self._L.idkptSynchronize(self._ctx))

    def download(self, which=0):
        out = np.zeros((self.rows, self.width, 4), np.float32)
        self._check(self._L.idkptDownload(self._ctx, which, out.ctypes.data, out.nbytes))
        return out

    def rays(self):
        out = np.zeros(self.rows * self.width, T.GpuWavefrontRay)
        self._check(self._L.idkptDownloadRays(self._ctx, out.ctypes.data, out.nbytes))
        return out

    def alive_queue(self):
        n = C.c_uint32()
        self._check(self._L.idkptDownloadAliveQueue(self._ctx, None, 0, C.byref(n)))
        out = np.zeros(n.value, np.uint32)
        if n.value:
            self._check(self._L.idkptDownloadAliveQueue(self._ctx, out.ctypes.data, n.value, C.byref(n)))
        return out

    def enable_primary_hit_capture(self, on=True):
        self._check(self._L.idkptEnablePrimaryHitCapture(self._ctx, 1 if on else 0))

    def primary_hits(self):
        n = self.rows * self.width
        t = np.zeros(n, np.float32); tri = np.zeros(n, np.uint32); bary = np.zeros((n, 2), np.float32)
        self._check(self._L.idkptDownloadPrimaryHits(self._ctx, t.ctypes.data, tri.ctypes.data, bary.ctypes.data, n))
        return t, tri, bary

    def tile_classes(self):
        """idkptDownloadTileClasses (a diagnostic): the classes of the 8x8 tiles of the last launched batch, a (sets, tilesY, tilesX) uint8 array — 0 per-pixel path, 1-6 proven
        miss + sky face, 7 proven miss without a sky, 8 proven miss under a textured sky; sets = 0 when that batch ran without a classification.  Member 0 of a multi-device context."""
        tx, ty, sets = C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self._L.idkptDownloadTileClasses(self._ctx, None, 0, C.byref(tx), C.byref(ty), C.byref(sets)))
        out = np.zeros((sets.value, ty.value, tx.value), np.uint8)
        if out.size:
            self._check(self._L.idkptDownloadTileClasses(self._ctx, out.ctypes.data, out.nbytes, C.byref(tx), C.byref(ty), C.byref(sets)))
        return out

    def UpdateTexture(self, index, image):
        """idkptUpdateTexture: image `index` of the texture table (a float32 array or a gputypes.TextureImage)."""
        t = T.TextureImage.of(image); rec = T.Texture(); t.fill(rec)
        self._check(self._L.idkptUpdateTexture(self._ctx, int(index), C.byref(rec)))

    def DownloadTexture(self, index):
        """idkptDownloadTexture: image `index` as the sampler sees it — (resident format, (h, w, 4) float32 array for RGBA32F, uint8 array for RGBA8 / SRGB8_A8)."""
        fmt, w, h = C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self._L.idkptDownloadTexture(self._ctx, int(index), C.byref(fmt), C.byref(w), C.byref(h), None, 0))
        out = np.zeros((h.value, w.value, 4), np.float32 if fmt.value == T.IDKPT_TEXFMT_RGBA32F else np.uint8)
        self._check(self._L.idkptDownloadTexture(self._ctx, int(index), C.byref(fmt), C.byref(w), C.byref(h), out.ctypes.data, out.nbytes))
        return fmt.value, out

    # ---- the sky without a scene upload (idkptComputeSky / idkptUpdateSky / idkptDownloadSky)
    def ComputeSky(self, size=128, atmosphere=None):
        """AtmosphericScatterer.Compute on the device: the six size x size faces of the procedural sky (gputypes.Atmosphere; default: the reference's 40, 8, 15, 0, 0)
        become the scene's sky.  Stream-ordered; the accumulation is the caller's to reset."""
        a = atmosphere if atmosphere is not None else T.Atmosphere()
        if not isinstance(a, T.Atmosphere):
            raise TypeError("ComputeSky: atmosphere must be a gputypes.Atmosphere")
        self._check(self._L.idkptComputeSky(self._ctx, int(size), C.addressof(a)))

    def UpdateSky(self, faces, format=T.IDKPT_TEXFMT_RGBA32F):
        """idkptUpdateSky: `faces` is None (no sky: black) or a C-contiguous (6, S, S, 4) array — float32 for IDKPT_TEXFMT_RGBA32F, uint8 for IDKPT_TEXFMT_RGBA8 /
        IDKPT_TEXFMT_SRGB8_A8 (face order +X, -X, +Y, -Y, +Z, -Z).  The array is checked against `format` here: the library only sees a pointer."""
        format = int(format)
        if format not in (T.IDKPT_TEXFMT_RGBA32F, T.IDKPT_TEXFMT_RGBA8, T.IDKPT_TEXFMT_SRGB8_A8):
            raise ValueError(f"UpdateSky: format {format} is not IDKPT_TEXFMT_RGBA32F, RGBA8 or SRGB8_A8")
        if faces is None:
            self._check(self._L.idkptUpdateSky(self._ctx, 0, format, None))
            return
        want = np.float32 if format == T.IDKPT_TEXFMT_RGBA32F else np.uint8
        if not isinstance(faces, np.ndarray) or faces.dtype != want:
            raise TypeError(f"UpdateSky: format {format} takes a {np.dtype(want).name} array, got {getattr(faces, 'dtype', type(faces).__name__)}")
        if faces.ndim != 4 or faces.shape[0] != 6 or faces.shape[3] != 4 or faces.shape[1] != faces.shape[2] or faces.shape[1] < 1:
            raise ValueError(f"UpdateSky: faces must have shape (6, S, S, 4), got {faces.shape}")
        if not faces.flags["C_CONTIGUOUS"]:
            raise ValueError("UpdateSky: faces must be C-contiguous (np.ascontiguousarray)")
        self._check(self._L.idkptUpdateSky(self._ctx, int(faces.shape[1]), format, faces.ctypes.data))

    def UnprojectSky(self, image, face_size=None):
        """idkptUnprojectSky (SkyBoxManager.LoadSkyBoxEquirectangular): `image` is the equirectangular panorama, a C-contiguous (H, W, 3) or (H, W, 4) float32 array, row 0
        the row GL receives first; face_size None = W // 4, as the reference sizes its cube map.  The faces are unprojected on the device and become the scene's sky; the
        call synchronises (load time).  A new environment invalidates what was accumulated: the accumulation is reset."""
        if not isinstance(image, np.ndarray) or image.dtype != np.float32:
            raise TypeError(f"UnprojectSky: image must be a float32 array, got {getattr(image, 'dtype', type(image).__name__)}")
        if image.ndim != 3 or image.shape[2] not in (3, 4) or image.shape[0] < 1 or image.shape[1] < 1:
            raise ValueError(f"UnprojectSky: image must have shape (H, W, 3) or (H, W, 4), got {image.shape}")
        if not image.flags["C_CONTIGUOUS"]:
            raise ValueError("UnprojectSky: image must be C-contiguous (np.ascontiguousarray)")
        self._check(self._L.idkptUnprojectSky(self._ctx, int(image.shape[1]), int(image.shape[0]), int(image.shape[2]), image.ctypes.data, 0 if face_size is None else int(face_size)))
        self.ResetAccumulation()

    def DownloadSky(self):
        """idkptDownloadSky: the resident faces, a (6, S, S, 4) float32 array (S = 0: no sky)."""
        s = C.c_int32()
        self._check(self._L.idkptDownloadSky(self._ctx, C.byref(s), None, 0))
        out = np.zeros((6, s.value, s.value, 4), np.float32)
        if s.value:
            self._check(self._L.idkptDownloadSky(self._ctx, C.byref(s), out.ctypes.data, out.nbytes))
        return out

    # ---- display output (idkptPresent / idkptDownloadDisplay / idkptGetDisplayDevicePtr): TonemapAndGammaCorrect.Compute on the device
    def _present(self, settings, image, slot, fmt, bloom=None):
        formats = {"rgba8": T.IDKPT_DISPLAY_RGBA8, "rgba32f": T.IDKPT_DISPLAY_RGBA32F}
        if fmt not in formats:
            raise ValueError(f"Present: fmt must be 'rgba8' or 'rgba32f', got {fmt!r}")
        if settings is None:
            settings = T.TonemapSettings(DoTonemapAndSrgbTransform=not self.DoDebugBVHTraversal)     # Application.cs:222
        if not isinstance(settings, T.TonemapSettings):
            raise TypeError("Present: settings must be a gputypes.TonemapSettings")
        slot = -1 if slot is None else int(slot)
        add0 = None
        if bloom is not None:                        # Application.cs:217-223: Bloom.Compute(Result), then TonemapAndGamma.Compute(Result, Bloom.Result)
            add0, _ = self.bloom_device_ptr(None if bloom is True else bloom, image, slot)
        self._check(self._L.idkptPresent(self._ctx, slot, int(image), C.addressof(settings), formats[fmt], add0, None))
        return slot, formats[fmt]

    def Present(self, settings=None, image=0, slot=None, fmt="rgba8", bloom=None):
        """TonemapAndGamma.Compute(PathTracer.Result) + the download of its R8G8B8A8Unorm result: the tone-mapped, sRGB-encoded, dithered image of `image` (0-2) of ring
        slot `slot` (None: the current one) as an (H, W, 4) numpy array of the presentation size (SetPresentationSize; the render size by default) — uint8 for fmt "rgba8", float32 (the value before quantisation) for "rgba32f".  settings: a
        gputypes.TonemapSettings; None = the reference's defaults with DoTonemapAndSrgbTransform = not DoDebugBVHTraversal, as Application.cs:222 sets it.
        bloom: None = no bloom (an unbound Sampler1); a gputypes.BloomSettings (or True: the reference's defaults) runs idkptBloom on the same image first and adds its
        expanded image as the shader's Sampler1, all on the device (one device, whole frame only)."""
        slot, f = self._present(settings, image, slot, fmt, bloom)
        out = np.zeros(self._display_shape() + (4,), np.float32 if f == T.IDKPT_DISPLAY_RGBA32F else np.uint8)
        self._check(self._L.idkptDownloadDisplay(self._ctx, slot, out.ctypes.data, out.nbytes))
        return out

    def present_device_ptr(self, settings=None, image=0, slot=None, fmt="rgba8", bloom=None):
        """idkptPresent + idkptGetDisplayDevicePtr: (device pointer, bytes) of the display image, valid in stream order; nothing is downloaded or waited for.  bloom: as Present."""
        slot, _ = self._present(settings, image, slot, fmt, bloom)
        p = C.c_void_p(); n = C.c_size_t()
        self._check(self._L.idkptGetDisplayDevicePtr(self._ctx, slot, C.byref(p), C.byref(n)))
        return p.value, n.value

    # ---- bloom (idkptBloom / idkptGetBloomInfo / idkptDownloadBloom / idkptGetBloomDevicePtr): Bloom.Compute on the device
    def bloom_device_ptr(self, settings=None, image=0, slot=None):
        """idkptBloom + idkptGetBloomDevicePtr: (device pointer, bytes) of the expanded RGBA32F image — idkptPresent's dAdd0 —, valid in stream order; nothing is waited for."""
        if settings is None:
            settings = T.BloomSettings()
        if not isinstance(settings, T.BloomSettings):
            raise TypeError("Bloom: settings must be a gputypes.BloomSettings")
        slot = -1 if slot is None else int(slot)
        self._check(self._L.idkptBloom(self._ctx, slot, int(image), C.addressof(settings)))
        p = C.c_void_p(); n = C.c_size_t()
        self._check(self._L.idkptGetBloomDevicePtr(self._ctx, slot, C.byref(p), C.byref(n)))
        return p.value, n.value

    def Bloom(self, settings=None, image=0, slot=None):
        """Bloom.Compute(image `image` (0-2) of ring slot `slot`; None: the current one) and what the tonemap shader reads of its result: the up chain's level 0 magnified to
        the frame, an (H, W, 4) float32 array (rgb, 1.0) of the presentation size.  settings: a gputypes.BloomSettings; None = the reference's defaults (1.5, 3.8, MinusLods 3)."""
        p, n = self.bloom_device_ptr(settings, image, slot)
        pw, ph = self.presentation_size
        out = np.zeros((ph, pw, 4), np.float32)
        if n != out.nbytes:
            raise IdkPtError(f"Bloom: the expanded image has {n} bytes, expected {out.nbytes} (height * width * 16)")
        self.read_device(p, out)
        return out

    def read_device(self, ptr, out):
        """Copies out.nbytes bytes at device pointer `ptr` (one the library returned for this context: image_device_ptr, present_device_ptr, bloom_device_ptr ...) into the
        C-contiguous numpy array `out`, ordered on the context's stream (idkptGetStream) behind what the library launched there; waits for the copy and returns `out`."""
        import torch                                   # (the plumbing: PyTorch-ROCm carries the copy; the stream is the library's)
        if not isinstance(out, np.ndarray) or not out.flags["C_CONTIGUOUS"]:
            raise ValueError("read_device: out must be a C-contiguous numpy array")
        st = C.c_void_p(); self._check(self._L.idkptGetStream(self._ctx, C.byref(st)))
        stream = torch.cuda.ExternalStream(st.value)
        holder = type("DevArray", (), {"__cuda_array_interface__": {"shape": (int(out.nbytes),), "typestr": "|u1", "data": (int(ptr), False), "version": 2}})()
        with torch.cuda.stream(stream):
            host = torch.as_tensor(holder, device="cuda").to("cpu")
        stream.synchronize()
        self._check(self._L.idkptSynchronize(self._ctx))   # (reports what the frame's kernels reported: a traversal stack overflow)
        out.view(np.uint8).reshape(-1)[:] = host.numpy()
        return out

    def bloom_info(self, slot=None):
        """idkptGetBloomInfo of the slot's last bloom: (levels, w0, h0)"""
        lv, w0, h0 = C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self._L.idkptGetBloomInfo(self._ctx, -1 if slot is None else int(slot), C.byref(lv), C.byref(w0), C.byref(h0)))
        return lv.value, w0.value, h0.value

    def bloom_chain_device_ptr(self, chain, slot=None):
        """idkptGetBloomChainDevicePtr: (device pointer, bytes) of the whole down (chain 0) or up (chain 1) chain of the slot's last bloom, level 0 first; 64 guard bytes follow"""
        p = C.c_void_p(); n = C.c_size_t()
        self._check(self._L.idkptGetBloomChainDevicePtr(self._ctx, -1 if slot is None else int(slot), int(chain), C.byref(p), C.byref(n)))
        return p.value, n.value

    def bloom_route(self, slot=None):
        """idkptGetBloomRoute of the slot's last bloom: gputypes.IDKPT_BLOOM_ROUTE_TILED or IDKPT_BLOOM_ROUTE_DIRECT (how down pass 0 read the image)"""
        r = C.c_int32()
        self._check(self._L.idkptGetBloomRoute(self._ctx, -1 if slot is None else int(slot), C.byref(r)))
        return r.value

    def bloom_level(self, chain, level, slot=None):
        """idkptDownloadBloom: level `level` of the down (chain 0) or up (chain 1) chain of the slot's last bloom, an (h, w, 4) float16 array (the stored RGBA16F bits)."""
        levels, w0, h0 = self.bloom_info(slot)
        if chain not in (0, 1) or not 0 <= int(level) < levels - chain:
            raise ValueError(f"bloom_level: chain {chain!r} level {level!r} outside the chains ({levels} down levels, {levels - 1} up levels)")
        out = np.zeros((max(h0 >> int(level), 1), max(w0 >> int(level), 1), 4), np.float16)
        self._check(self._L.idkptDownloadBloom(self._ctx, -1 if slot is None else int(slot), int(chain), int(level), out.ctypes.data, out.nbytes))
        return out

    # ---- denoised output (idkptDenoise / idkptUploadDenoised / idkptDownloadDenoised / idkptSetResultSource): PathTracerPipeline.Result == Denoised
    def Denoise(self, settings=None, slot=None):
        """idkptDenoise + idkptDownloadDenoised: the edge-avoiding a-trous filter of include/idkpt.h over Result, guided by Albedo and Normal of ring slot `slot` (None: the
        current one; needs OutputAOVs), as an (H, W, 4) float32 array (rgb, 1.0).  settings: a gputypes.Denoise; None = the tuned defaults.  The image stays in the slot:
        with SetResultSource(IDKPT_RESULT_DENOISED), Present and Bloom read it in place of image 0.  Not OIDN and no approximation of it."""
        if settings is None:
            settings = T.Denoise()
        if not isinstance(settings, T.Denoise):
            raise TypeError("Denoise: settings must be a gputypes.Denoise")
        slot = -1 if slot is None else int(slot)
        self._check(self._L.idkptDenoise(self._ctx, slot, C.addressof(settings)))
        return self.DownloadDenoised(slot)

    def DenoiseVariance(self, settings=None, slot=None):
        """idkptDenoiseVariance + idkptDownloadDenoised: the variance-guided a-trous filter of include/idkpt.h over Result of ring slot `slot` (None: the current one), guided
        by Albedo, Normal and the luminance moments (needs OutputAOVs, SetNoiseEstimate(True) and 2 accumulated samples), as an (H, W, 4) float32 array (rgb, 1.0).
        settings: a gputypes.DenoiseVariance; None = the defaults.  It fills the image Denoise fills: Present and Bloom read it under IDKPT_RESULT_DENOISED."""
        if settings is None:
            settings = T.DenoiseVariance()
        if not isinstance(settings, T.DenoiseVariance):
            raise TypeError("DenoiseVariance: settings must be a gputypes.DenoiseVariance")
        slot = -1 if slot is None else int(slot)
        self._check(self._L.idkptDenoiseVariance(self._ctx, slot, C.addressof(settings)))
        return self.DownloadDenoised(slot)

    def UploadDenoised(self, rgba, slot=None):
        """idkptUploadDenoised: the host's own denoiser's output, an (H, W, 4) float32 array, becomes the denoised image of the slot (the reference's denoisedTexture.Upload2D)"""
        rgba = np.ascontiguousarray(rgba, np.float32)
        if rgba.shape != (self.height, self.width, 4):
            raise ValueError(f"UploadDenoised: expected an array of shape {(self.height, self.width, 4)}, got {rgba.shape}")
        self._check(self._L.idkptUploadDenoised(self._ctx, -1 if slot is None else int(slot), rgba.ctypes.data, rgba.nbytes))

    def DownloadDenoised(self, slot=None):
        """idkptDownloadDenoised: the denoised image of the slot, an (H, W, 4) float32 array"""
        out = np.zeros((self.height, self.width, 4), np.float32)
        self._check(self._L.idkptDownloadDenoised(self._ctx, -1 if slot is None else int(slot), out.ctypes.data, out.nbytes))
        return out

    def denoised_device_ptr(self, slot=None):
        """idkptGetDenoisedDevicePtr: (device pointer, bytes) of the slot's denoised image, valid in stream order; 64 guard bytes follow"""
        p = C.c_void_p(); n = C.c_size_t()
        self._check(self._L.idkptGetDenoisedDevicePtr(self._ctx, -1 if slot is None else int(slot), C.byref(p), C.byref(n)))
        return p.value, n.value

    def denoise_route(self, iteration, slot=None):
        """idkptGetDenoiseRoute: gputypes.IDKPT_DENOISE_ROUTE_TILED or IDKPT_DENOISE_ROUTE_DIRECT for an iteration of the slot's last Denoise"""
        r = C.c_int32()
        self._check(self._L.idkptGetDenoiseRoute(self._ctx, -1 if slot is None else int(slot), int(iteration), C.byref(r)))
        return r.value

    def SetResultSource(self, source):
        """idkptSetResultSource: gputypes.IDKPT_RESULT_NOISY (default) or IDKPT_RESULT_DENOISED — what image 0 means to Present and Bloom (PathTracerPipeline.Result's switch).
        A state of its own: ResetAccumulation does not revert it."""
        self._check(self._L.idkptSetResultSource(self._ctx, int(source)))

    def GetResultSource(self):
        s = C.c_int32()
        self._check(self._L.idkptGetResultSource(self._ctx, C.byref(s)))
        return s.value

    # ---- noise estimate (idkptSetNoiseEstimate / idkptEstimateNoise / idkptDownloadNoise / idkptDownloadMoments): no counterpart in the reference
    def SetNoiseEstimate(self, enable):
        """idkptSetNoiseEstimate: while on, FinalDraw keeps the luminance moments (m1, m2) of every pixel beside the running mean.  Changing the value launches the queued
        samples and restarts the accumulation.  One device that holds the whole frame."""
        self._check(self._L.idkptSetNoiseEstimate(self._ctx, 1 if enable else 0))

    def GetNoiseEstimate(self):
        e = C.c_int32()
        self._check(self._L.idkptGetNoiseEstimate(self._ctx, C.byref(e)))
        return bool(e.value)

    def EstimateNoise(self, settings=None, slot=None):
        """idkptEstimateNoise + idkptDownloadNoise: the relative standard error of the mean luminance per 8 x 8 tile of ring slot `slot` (None: the current one) as a
        (tilesY, tilesX, 2) float32 array of (mean, max), and the summary as a dict.  settings: a gputypes.Noise; None = the (untuned) defaults.  Needs 2 samples."""
        if settings is None:
            settings = T.Noise()
        if not isinstance(settings, T.Noise):
            raise TypeError("EstimateNoise: settings must be a gputypes.Noise")
        slot = -1 if slot is None else int(slot)
        self._check(self._L.idkptEstimateNoise(self._ctx, slot, C.addressof(settings)))
        return self.DownloadNoise(slot)

    def DownloadNoise(self, slot=None):
        """idkptDownloadNoise: (tiles, summary) of the slot's last EstimateNoise"""
        tiles = np.zeros(((self.height + 7) // 8, (self.width + 7) // 8, 2), np.float32)
        s = T.NoiseSummary()
        self._check(self._L.idkptDownloadNoise(self._ctx, -1 if slot is None else int(slot), tiles.ctypes.data, tiles.nbytes, C.addressof(s)))
        return tiles, {"TilesAbove": s.TilesAbove, "MaxTileMean": s.MaxTileMean, "Tiles": s.Tiles, "Samples": s.Samples}

    def DownloadMoments(self, slot=None):
        """idkptDownloadMoments: the moments image of the slot, an (H, W, 4) float32 array of (m1, m2, 0, 1)"""
        out = np.zeros((self.height, self.width, 4), np.float32)
        self._check(self._L.idkptDownloadMoments(self._ctx, -1 if slot is None else int(slot), out.ctypes.data, out.nbytes))
        return out

    def noise_device_ptrs(self, slot=None):
        """idkptGetNoiseDevicePtr: (tile map pointer, summary pointer, tile map bytes), valid in stream order; 64 guard bytes follow each"""
        t = C.c_void_p(); s = C.c_void_p(); n = C.c_size_t()
        self._check(self._L.idkptGetNoiseDevicePtr(self._ctx, -1 if slot is None else int(slot), C.byref(t), C.byref(s), C.byref(n)))
        return t.value, s.value, n.value

    def moments_device_ptr(self, slot=None):
        """idkptGetMomentsDevicePtr: (device pointer, bytes) of the slot's moments image, valid in stream order; 64 guard bytes follow"""
        p = C.c_void_p(); n = C.c_size_t()
        self._check(self._L.idkptGetMomentsDevicePtr(self._ctx, -1 if slot is None else int(slot), C.byref(p), C.byref(n)))
        return p.value, n.value

    # ---- temporal reprojection (idkptCaptureGeometry / idkptReproject / idkptUseTemporalAsDenoised / idkptSetDenoiseInput): no counterpart in the reference
    def CaptureGeometry(self, slot=None):
        """idkptCaptureGeometry: one centre ray per pixel under the current camera -> the geometry image of ring slot `slot` (None: the current one)"""
        self._check(self._L.idkptCaptureGeometry(self._ctx, -1 if slot is None else int(slot)))

    def DownloadGeometry(self, slot=None):
        """idkptDownloadGeometry: (H, W, 4) float32 — the world position of the pixel centre's hit and the bits of its MeshTransformId, or the ray direction and 0xFFFFFFFF"""
        out = np.zeros((self.height, self.width, 4), np.float32)
        self._check(self._L.idkptDownloadGeometry(self._ctx, -1 if slot is None else int(slot), out.ctypes.data, out.nbytes))
        return out

    def Reproject(self, slot=None, history=T.IDKPT_NO_HISTORY, settings=None):
        """idkptReproject: blends Result of `slot` with the temporal image of ring slot `history` found through that frame's camera (settings: a gputypes.Reproject holding
        its PrevProjView and PrevViewPos); history = IDKPT_NO_HISTORY starts a history.  Both slots need CaptureGeometry first.  The result stays in the slot's temporal
        image (DownloadTemporal)."""
        if settings is None:
            settings = T.Reproject()
        if not isinstance(settings, T.Reproject):
            raise TypeError("Reproject: settings must be a gputypes.Reproject")
        self._check(self._L.idkptReproject(self._ctx, -1 if slot is None else int(slot), int(history), C.addressof(settings)))

    def DownloadTemporal(self, slot=None):
        """idkptDownloadTemporal: (H, W, 4) float32 — rgb and the effective sample count"""
        out = np.zeros((self.height, self.width, 4), np.float32)
        self._check(self._L.idkptDownloadTemporal(self._ctx, -1 if slot is None else int(slot), out.ctypes.data, out.nbytes))
        return out

    def geometry_device_ptr(self, slot=None):
        """idkptGetGeometryDevicePtr: (device pointer, bytes), valid in stream order; 64 guard bytes follow"""
        p = C.c_void_p(); n = C.c_size_t()
        self._check(self._L.idkptGetGeometryDevicePtr(self._ctx, -1 if slot is None else int(slot), C.byref(p), C.byref(n)))
        return p.value, n.value

    def temporal_device_ptr(self, slot=None):
        """idkptGetTemporalDevicePtr: (device pointer, bytes), valid in stream order; 64 guard bytes follow"""
        p = C.c_void_p(); n = C.c_size_t()
        self._check(self._L.idkptGetTemporalDevicePtr(self._ctx, -1 if slot is None else int(slot), C.byref(p), C.byref(n)))
        return p.value, n.value

    def UseTemporalAsDenoised(self, slot=None):
        """idkptUseTemporalAsDenoised: the slot's temporal rgb (alpha 1.0) becomes its denoised image; Present and Bloom show it under IDKPT_RESULT_DENOISED"""
        self._check(self._L.idkptUseTemporalAsDenoised(self._ctx, -1 if slot is None else int(slot)))

    def SetDenoiseInput(self, source):
        """idkptSetDenoiseInput: gputypes.IDKPT_DENOISE_INPUT_ACCUMULATED (default) or IDKPT_DENOISE_INPUT_TEMPORAL — where Denoise takes its colour from"""
        self._check(self._L.idkptSetDenoiseInput(self._ctx, int(source)))

    def GetDenoiseInput(self):
        s = C.c_int32()
        self._check(self._L.idkptGetDenoiseInput(self._ctx, C.byref(s)))
        return s.value

    # ---- temporal moments (idkptReprojectMoments / idkptDenoiseTemporal): the variance-guided filter on the reprojected frame; no counterpart in the reference
    def ReprojectMoments(self, slot=None, history=T.IDKPT_NO_HISTORY, settings=None):
        """idkptReprojectMoments: blends the luminance moments of `slot` (SetNoiseEstimate(True)) with the temporal moments image of ring slot `history` through the taps of
        Reproject (settings: the same gputypes.Reproject); history = IDKPT_NO_HISTORY starts a history.  Both slots need CaptureGeometry first.  The result stays in the
        slot's temporal moments image (DownloadTemporalMoments)."""
        if settings is None:
            settings = T.Reproject()
        if not isinstance(settings, T.Reproject):
            raise TypeError("ReprojectMoments: settings must be a gputypes.Reproject")
        self._check(self._L.idkptReprojectMoments(self._ctx, -1 if slot is None else int(slot), int(history), C.addressof(settings)))

    def DownloadTemporalMoments(self, slot=None):
        """idkptDownloadTemporalMoments: (H, W, 4) float32 — (M1, M2, 0, the effective sample count)"""
        out = np.zeros((self.height, self.width, 4), np.float32)
        self._check(self._L.idkptDownloadTemporalMoments(self._ctx, -1 if slot is None else int(slot), out.ctypes.data, out.nbytes))
        return out

    def temporal_moments_device_ptr(self, slot=None):
        """idkptGetTemporalMomentsDevicePtr: (device pointer, bytes), valid in stream order; 64 guard bytes follow"""
        p = C.c_void_p(); n = C.c_size_t()
        self._check(self._L.idkptGetTemporalMomentsDevicePtr(self._ctx, -1 if slot is None else int(slot), C.byref(p), C.byref(n)))
        return p.value, n.value

    def DenoiseTemporal(self, settings=None, slot=None):
        """idkptDenoiseTemporal + idkptDownloadDenoised: the variance-guided a-trous filter over the TEMPORAL image of ring slot `slot` (None: the current one), its variance
        from the slot's temporal moments image (needs OutputAOVs, Reproject and ReprojectMoments), as an (H, W, 4) float32 array (rgb, 1.0).  settings: a
        gputypes.DenoiseTemporal; None = the defaults.  It fills the image Denoise fills: Present and Bloom read it under IDKPT_RESULT_DENOISED."""
        if settings is None:
            settings = T.DenoiseTemporal()
        if not isinstance(settings, T.DenoiseTemporal):
            raise TypeError("DenoiseTemporal: settings must be a gputypes.DenoiseTemporal")
        slot = -1 if slot is None else int(slot)
        self._check(self._L.idkptDenoiseTemporal(self._ctx, slot, C.addressof(settings)))
        return self.DownloadDenoised(slot)

    # ---- motion-aware capture (idkptCaptureMotion): reprojection that follows moving objects; the reference's path tracer has no counterpart
    def CaptureMotion(self, slot=None):
        """idkptCaptureMotion: CaptureGeometry plus the slot's motion image — where each pixel's surface point stood in the previous frame (the previous vertex positions
        through PrevModel).  Reproject / ReprojectMoments of a slot that holds one look the history up there.  CaptureGeometry on the slot drops it."""
        self._check(self._L.idkptCaptureMotion(self._ctx, -1 if slot is None else int(slot)))

    def DownloadMotion(self, slot=None):
        """idkptDownloadMotion: (H, W, 4) float32 — the previous world position of the pixel centre's hit and the bits of its MeshTransformId, or the geometry record of a miss"""
        out = np.zeros((self.height, self.width, 4), np.float32)
        self._check(self._L.idkptDownloadMotion(self._ctx, -1 if slot is None else int(slot), out.ctypes.data, out.nbytes))
        return out

    def motion_device_ptr(self, slot=None):
        """idkptGetMotionDevicePtr: (device pointer, bytes), valid in stream order; 64 guard bytes follow"""
        p = C.c_void_p(); n = C.c_size_t()
        self._check(self._L.idkptGetMotionDevicePtr(self._ctx, -1 if slot is None else int(slot), C.byref(p), C.byref(n)))
        return p.value, n.value

    def DownloadMotionPrevPositions(self, count):
        """IDKPT_BUF_MOTION_PREV_POSITIONS: (count, 3) float32 — the local positions the first `count` vertices had before the last Skin that wrote them (the positions
        themselves where none did); raises before the context's first CaptureMotion"""
        return self.DownloadBuffer(T.IDKPT_BUF_MOTION_PREV_POSITIONS, np.float32, int(count) * 3).reshape(-1, 3)

    # ---- history rectification (idkptReprojectFast / idkptRectifyHistory): a fast history that ends lag after lighting changes; no counterpart in the reference
    def ReprojectFast(self, slot=None, history=T.IDKPT_NO_HISTORY, settings=None):
        """idkptReprojectFast: Reproject on the slot's FAST temporal image and the fast temporal image of ring slot `history` (settings: a gputypes.Reproject whose
        MaxHistory is the fast cap; None: the defaults with MaxHistory = 4); history = IDKPT_NO_HISTORY starts it.  The result stays in the slot's fast temporal image
        (DownloadFastTemporal)."""
        if settings is None:
            settings = T.Reproject(MaxHistory=4.0)
        if not isinstance(settings, T.Reproject):
            raise TypeError("ReprojectFast: settings must be a gputypes.Reproject")
        self._check(self._L.idkptReprojectFast(self._ctx, -1 if slot is None else int(slot), int(history), C.addressof(settings)))

    def DownloadFastTemporal(self, slot=None):
        """idkptDownloadFastTemporal: (H, W, 4) float32 — rgb and the effective sample count of the fast history"""
        out = np.zeros((self.height, self.width, 4), np.float32)
        self._check(self._L.idkptDownloadFastTemporal(self._ctx, -1 if slot is None else int(slot), out.ctypes.data, out.nbytes))
        return out

    def fast_temporal_device_ptr(self, slot=None):
        """idkptGetFastTemporalDevicePtr: (device pointer, bytes), valid in stream order; 64 guard bytes follow"""
        p = C.c_void_p(); n = C.c_size_t()
        self._check(self._L.idkptGetFastTemporalDevicePtr(self._ctx, -1 if slot is None else int(slot), C.byref(p), C.byref(n)))
        return p.value, n.value

    def RectifyHistory(self, settings=None, slot=None):
        """idkptRectifyHistory: where the slot's fast and long history disagree by more than their noise explains, its temporal image and sample count (and the count of
        its temporal moments image) are pulled towards the fast temporal image.  Needs CaptureGeometry, Reproject and ReprojectFast of the slot.  settings: a
        gputypes.Rectify; None = the defaults.  The temporal image moves to another buffer: ask temporal_device_ptr again afterwards."""
        if settings is None:
            settings = T.Rectify()
        if not isinstance(settings, T.Rectify):
            raise TypeError("RectifyHistory: settings must be a gputypes.Rectify")
        self._check(self._L.idkptRectifyHistory(self._ctx, -1 if slot is None else int(slot), C.addressof(settings)))

    # ---- history reconstruction (idkptReconstructHistory): disoccluded pixels filled from their neighbours; no counterpart in the reference
    def ReconstructHistory(self, slot=-1, **settings):
        """idkptReconstructHistory: the pixels of the slot's temporal image whose count is below FillBelow take colour from texels of the same surface that kept their
        history, in place (temporal_device_ptr stays valid; the counts, the temporal moments and the fast temporal image are untouched).  Needs CaptureGeometry and
        Reproject of the slot and OutputAOVs.  Call it behind Reproject / ReprojectMoments / ReprojectFast and before RectifyHistory and DenoiseTemporal.  settings: the
        fields of gputypes.Reconstruct (Radius, Stride, FillBelow, AlbedoSigma, NormalSigma); those not given keep their defaults."""
        s = T.Reconstruct(**settings)
        self._check(self._L.idkptReconstructHistory(self._ctx, int(slot), C.addressof(s)))

    def enable_counters(self, on=True):
        self._check(self._L.idkptEnableCounters(self._ctx, 1 if on else 0))

    def enable_timing(self, on=True):
        self._check(self._L.idkptEnableTiming(self._ctx, 1 if on else 0))

    def stats(self):
        s = T.Stats()
        self._check(self._L.idkptGetStatsSized(self._ctx, C.addressof(s), C.sizeof(s)))
        return {"rays_traced": s.RaysTraced, "primary_rays": s.PrimaryRays, "frames": s.Frames, "alive_counts": list(s.LastAliveCounts),
                "last_frame_ms": s.LastFrameMs, "node_pair_visits": s.NodePairVisits, "triangle_tests": s.TriangleTests,
                "trace_ms_total": s.TraceMsTotal, "trace_launches": s.TraceLaunches,
                "wide_flagged_rays": s.WideFlaggedRays, "wide_node_visits": s.WideNodeVisits, "wide_leaf_records": s.WideLeafRecords, "wide_triangle_tests": s.WideTriangleTests,
                "inst_tlas_flagged_rays": s.InstTlasFlaggedRays,
                "packet_flagged_rays": s.PacketFlaggedRays, "packet_packets": s.PacketPackets, "packet_node_steps": s.PacketNodeSteps, "packet_live_lanes": s.PacketLiveLanes,
                "packet_rays_entered": s.PacketRaysEntered, "packet_triangle_rounds": s.PacketTriangleRounds,
                "inst_unified_launches": s.InstUnifiedLaunches, "inst_unified_entries": s.InstUnifiedEntries, "inst_unified_top_depth": s.InstUnifiedTopDepth,
                "last_occlusion_launches": s.LastOcclusionLaunches, "last_fold_batches": s.LastFoldBatches}

    def reset_stats(self):
        self._check(self._L.idkptResetStats(self._ctx))

    def image_device_ptr(self, which=0):
        p = C.c_void_p(); n = C.c_size_t()
        self._check(self._L.idkptGetImageDevicePtr(self._ctx, which, C.byref(p), C.byref(n)))
        return p.value, n.value

    # ---- frame ring: several frames (cameras) in flight, idkptSetFrameRing / idkptBeginFrame / idkptDownloadFrame
    def SetFrameRing(self, frames):
        self._check(self._L.idkptSetFrameRing(self._ctx, int(frames)))

    def BeginFrame(self):
        """The next ring slot becomes current (accumulation restarts); returns the slot to read the finished frame from later."""
        slot = C.c_int32()
        self._check(self._L.idkptBeginFrame(self._ctx, C.byref(slot)))
        return slot.value

    def FrameResult(self, slot, which=0):
        out = np.zeros((self.rows, self.width, 4), np.float32)
        self._check(self._L.idkptDownloadFrame(self._ctx, int(slot), which, out.ctypes.data, out.nbytes))
        return out

    def frame_device_ptr(self, slot, which=0):
        p = C.c_void_p(); n = C.c_size_t()
        self._check(self._L.idkptGetFrameDevicePtr(self._ctx, int(slot), which, C.byref(p), C.byref(n)))
        return p.value, n.value

    def set_max_batch(self, n):
        """Up to n consecutive samples are deferred and traced together (bit-identical results; idkptSetMaxBatch)."""
        self._check(self._L.idkptSetMaxBatch(self._ctx, n))

    def flush(self):
        self._check(self._L.idkptFlush(self._ctx))

    def set_option(self, name, value):
        """idkptSetDeveloperOption: tuning / test hooks (include/idkpt.h); results are bit-identical under all of them."""
        self._check(self._L.idkptSetDeveloperOption(self._ctx, name.encode(), int(value)))

    def set_stream(self, hip_stream_handle):
        self._check(self._L.idkptSetStream(self._ctx, C.c_void_p(hip_stream_handle)))
