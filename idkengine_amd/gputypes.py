"""numpy mirrors of include/idkpt_types.h (byte-exact; sizes asserted at import).

Reference: IDKEngine/Source/GpuTypes/*.cs <-> IDKEngine/Resource/Shaders/include/GpuTypes.glsl.
"""
import ctypes as C
import numpy as np

GpuBlasNode = np.dtype([("Min", "<f4", 3), ("TriStartOrChild", "<u4"), ("Max", "<f4", 3), ("TriCount", "<u4")])
GpuBlasTriangle = np.dtype([("X", "<u4"), ("Y", "<u4"), ("Z", "<u4"), ("MeshId", "<u4")])
GpuBlasDesc = np.dtype([
    ("NodeOffset", "<i4"), ("NodeCount", "<i4"), ("TriangleOffset", "<i4"), ("TriangleCount", "<i4"),
    ("LeafIndicesOffset", "<i4"), ("LeafIndicesCount", "<i4"), ("ParentIndicesOffset", "<i4"), ("ParentIndicesCount", "<i4"),
    ("RequiredStackSize", "<i4"), ("IsRefittable", "u1"), ("_pad", "u1", 3)])
GpuBlasInstance = np.dtype([("BlasId", "<u4"), ("MeshTransformId", "<u4")])
GpuTlasNode = np.dtype([("Min", "<f4", 3), ("IsLeafAndChildOrInstanceId", "<u4"), ("Max", "<f4", 3), ("_pad0", "<f4")])
GpuMeshTransform = np.dtype([("Model", "<f4", (3, 4)), ("InvModel", "<f4", (3, 4)), ("PrevModel", "<f4", (3, 4))])
GpuMesh = np.dtype([
    ("LocalBoundsMin", "<f4", 3), ("MaterialId", "<i4"), ("LocalBoundsMax", "<f4", 3), ("NormalMapStrength", "<f4"),
    ("AbsorbanceBias", "<f4", 3), ("MeshletsOffset", "<i4"), ("MeshletCount", "<i4"), ("EmissiveBias", "<f4"),
    ("SpecularBias", "<f4"), ("RoughnessBias", "<f4"), ("TransmissionBias", "<f4"), ("IORBias", "<f4"),
    ("InstanceCount", "<i4"), ("VertexCount", "<i4"), ("_pad0", "<f4", 3), ("TintOnTransmissive", "u1"), ("_pad1", "u1", 3)])
GpuMaterial = np.dtype([
    ("EmissiveFactor", "<f4", 3), ("BaseColorFactor", "<u4"), ("Absorbance", "<f4", 3), ("IOR", "<f4"),
    ("TransmissionFactor", "<f4"), ("RoughnessFactor", "<f4"), ("MetallicFactor", "<f4"), ("AlphaCutoff", "<f4"),
    ("BaseColorTexture", "<u8"), ("MetallicRoughnessTexture", "<u8"), ("NormalTexture", "<u8"), ("EmissiveTexture", "<u8"),
    ("TransmissionTexture", "<u8"), ("IsVolumetric", "u1"), ("_pad0", "u1", 3), ("IsDoubleSided", "u1"), ("_pad1", "u1", 3)])
GpuVertex = np.dtype([("TexCoord", "<f4", 2), ("Tangent", "<u4"), ("Normal", "<u4")])
GpuLight = np.dtype([("Position", "<f4", 3), ("Radius", "<f4"), ("Color", "<f4", 3), ("PointShadowIndex", "<i4"),
                     ("PrevPosition", "<f4", 3), ("_pad0", "<f4")])
GpuWavefrontRay = np.dtype([("Origin", "<f4", 3), ("PreviousIOROrTraverseCost", "<f4"), ("Throughput", "<f4", 3),
                            ("PackedDirectionX", "<f4"), ("Radiance", "<f4", 3), ("PackedDirectionY", "<f4")])
GpuUnskinnedVertex = np.dtype([("JointIndices", "<u4", 4), ("JointWeights", "<f4", 4), ("Position", "<f4", 3),
                               ("Tangent", "<u4"), ("Normal", "<u4")])

for _dt, _sz in ((GpuBlasNode, 32), (GpuBlasTriangle, 16), (GpuBlasDesc, 40), (GpuBlasInstance, 8), (GpuTlasNode, 32),
                 (GpuMeshTransform, 144), (GpuMesh, 96), (GpuMaterial, 96), (GpuVertex, 16), (GpuLight, 48),
                 (GpuWavefrontRay, 48), (GpuUnskinnedVertex, 52)):
    assert _dt.itemsize == _sz, (_dt, _dt.itemsize, _sz)


class GpuSettings(C.Structure):
    """PathTracer.GpuSettings (Source/Render/PathTracer.cs:127-138)."""
    _fields_ = [("FocalLength", C.c_float), ("LenseRadius", C.c_float), ("DoDebugBVHTraversal", C.c_int32),
                ("DoTraceLights", C.c_int32), ("DoRussianRoulette", C.c_int32)]


class Settings(C.Structure):
    """idkpt_settings (include/idkpt.h)."""
    _fields_ = [("Gpu", GpuSettings), ("RayDepth", C.c_int32), ("SamplesPerPixel", C.c_int32), ("DoRaySorting", C.c_int32),
                ("OutputAOVs", C.c_int32), ("UseTlas", C.c_int32), ("BlasStackSize", C.c_int32)]

    @staticmethod
    def default():
        s = Settings()
        s.Gpu.FocalLength = 8.0
        s.Gpu.LenseRadius = 0.0
        s.Gpu.DoDebugBVHTraversal = 0
        s.Gpu.DoTraceLights = 0
        s.Gpu.DoRussianRoulette = 1
        s.RayDepth = 7
        s.SamplesPerPixel = 1
        s.DoRaySorting = 0
        s.OutputAOVs = 0
        s.UseTlas = 0
        s.BlasStackSize = 0
        return s


class Texture(C.Structure):
    """idkpt_texture (include/idkpt.h), 32 bytes."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("rgba", C.c_void_p), ("wrapS", C.c_int32), ("wrapT", C.c_int32), ("magFilter", C.c_int32), ("format", C.c_int32)]


# enum idkpt_wrap / idkpt_filter / idkpt_texture_format
IDKPT_WRAP_REPEAT, IDKPT_WRAP_CLAMP_TO_EDGE, IDKPT_WRAP_MIRRORED_REPEAT = range(3)
IDKPT_FILTER_LINEAR, IDKPT_FILTER_NEAREST = range(2)
(IDKPT_TEXFMT_RGBA32F, IDKPT_TEXFMT_RGBA8, IDKPT_TEXFMT_SRGB8_A8, IDKPT_TEXFMT_R8, IDKPT_TEXFMT_RG8, IDKPT_TEXFMT_R11G11B10F, IDKPT_TEXFMT_BC4_R, IDKPT_TEXFMT_BC5_RG,
 IDKPT_TEXFMT_BC7_RGBA, IDKPT_TEXFMT_BC7_SRGBA) = range(10)
# source formats (>= IDKPT_TEXFMT_R8, decoded on the device at upload) -> the resident format the sampler reads
TEXFMT_RESIDENT = {IDKPT_TEXFMT_R8: IDKPT_TEXFMT_RGBA8, IDKPT_TEXFMT_RG8: IDKPT_TEXFMT_RGBA8, IDKPT_TEXFMT_R11G11B10F: IDKPT_TEXFMT_RGBA32F, IDKPT_TEXFMT_BC4_R: IDKPT_TEXFMT_RGBA32F,
                   IDKPT_TEXFMT_BC5_RG: IDKPT_TEXFMT_RGBA32F, IDKPT_TEXFMT_BC7_RGBA: IDKPT_TEXFMT_RGBA8, IDKPT_TEXFMT_BC7_SRGBA: IDKPT_TEXFMT_SRGB8_A8}


def texture_storage_bytes(format, width, height):
    """Bytes a host passes for a width x height image of `format` (the table of include/idkpt.h)."""
    texels, blocks = width * height, ((width + 3) // 4) * ((height + 3) // 4)
    return {IDKPT_TEXFMT_RGBA32F: texels * 16, IDKPT_TEXFMT_RGBA8: texels * 4, IDKPT_TEXFMT_SRGB8_A8: texels * 4, IDKPT_TEXFMT_R8: texels, IDKPT_TEXFMT_RG8: texels * 2,
            IDKPT_TEXFMT_R11G11B10F: texels * 4, IDKPT_TEXFMT_BC4_R: blocks * 8, IDKPT_TEXFMT_BC5_RG: blocks * 16, IDKPT_TEXFMT_BC7_RGBA: blocks * 16, IDKPT_TEXFMT_BC7_SRGBA: blocks * 16}[format]
GL_WRAP = {0x2901: IDKPT_WRAP_REPEAT, 0x812F: IDKPT_WRAP_CLAMP_TO_EDGE, 0x8370: IDKPT_WRAP_MIRRORED_REPEAT}      # GLSampler.WrapMode (glTF sampler.wrapS / wrapT) -> enum idkpt_wrap
GL_MAG_FILTER = {0x2601: IDKPT_FILTER_LINEAR, 0x2600: IDKPT_FILTER_NEAREST}                                       # GLSampler.MagFilter -> enum idkpt_filter


class TextureImage:
    """One image of the texture table with its sampler state: what a GpuMaterial handle stands for in the reference (a bindless texture + the GLSampler.SamplerState of
    Utils/ModelLoader.cs:1166-1197).  data: (h, w, 4) float32 (RGBA32F) or uint8 (RGBA8 / SRGB8_A8).  A bare float32 array in Scene.textures means REPEAT / REPEAT / LINEAR."""

    def __init__(self, data, wrap_s=IDKPT_WRAP_REPEAT, wrap_t=IDKPT_WRAP_REPEAT, mag_filter=IDKPT_FILTER_LINEAR, srgb=False):
        data = np.asarray(data)
        if data.dtype == np.uint8:
            self.data = np.ascontiguousarray(data); self.format = IDKPT_TEXFMT_SRGB8_A8 if srgb else IDKPT_TEXFMT_RGBA8
        else:
            assert not srgb, "sRGB storage is 8-bit"
            self.data = np.ascontiguousarray(data, np.float32); self.format = IDKPT_TEXFMT_RGBA32F
        assert self.data.ndim == 3 and self.data.shape[2] == 4
        self.wrap_s, self.wrap_t, self.mag_filter = int(wrap_s), int(wrap_t), int(mag_filter)

    _size = None    # (width, height) of a from_storage image; otherwise the array's shape says it

    @property
    def width(self):
        return self._size[0] if self._size else self.data.shape[1]

    @property
    def height(self):
        return self._size[1] if self._size else self.data.shape[0]

    @staticmethod
    def from_storage(format, width, height, data, wrap_s=IDKPT_WRAP_REPEAT, wrap_t=IDKPT_WRAP_REPEAT, mag_filter=IDKPT_FILTER_LINEAR):
        """An image in one of the storage formats the library decodes on the device (IDKPT_TEXFMT_R8 .. IDKPT_TEXFMT_BC7_SRGBA): `data` is the bytes as the engine holds them —
        any array or buffer of exactly texture_storage_bytes(format, width, height) bytes (tightly packed rows, or 4x4 blocks row-major over the block grid)."""
        format, width, height = int(format), int(width), int(height)
        assert format in TEXFMT_RESIDENT, "from_storage is for the formats decoded on the device; RGBA32F / RGBA8 / SRGB8_A8 images are made by the constructor"
        assert width > 0 and height > 0
        t = TextureImage.__new__(TextureImage)
        t.data = np.ascontiguousarray(np.frombuffer(np.ascontiguousarray(data).tobytes(), np.uint8))
        assert t.data.nbytes == texture_storage_bytes(format, width, height), (t.data.nbytes, texture_storage_bytes(format, width, height))
        t.format, t._size = format, (width, height)
        t.wrap_s, t.wrap_t, t.mag_filter = int(wrap_s), int(wrap_t), int(mag_filter)
        return t

    @staticmethod
    def of(t):
        return t if isinstance(t, TextureImage) else TextureImage(t)

    def fill(self, rec):
        """Writes this image into a Texture record; the record borrows self.data."""
        rec.height, rec.width, rec.rgba = self.height, self.width, self.data.ctypes.data
        rec.wrapS, rec.wrapT, rec.magFilter, rec.format = self.wrap_s, self.wrap_t, self.mag_filter, self.format


class SceneDesc(C.Structure):
    """idkpt_scene_desc (include/idkpt.h)."""
    _fields_ = [
        ("BlasNodes", C.c_void_p), ("BlasNodeCount", C.c_int32),
        ("BlasTriangles", C.c_void_p), ("BlasTriangleCount", C.c_int32),
        ("BlasDescs", C.c_void_p), ("BlasDescCount", C.c_int32),
        ("BlasInstances", C.c_void_p), ("BlasInstanceCount", C.c_int32),
        ("TlasNodes", C.c_void_p), ("TlasNodeCount", C.c_int32),
        ("BlasParentIndices", C.c_void_p), ("BlasParentIndexCount", C.c_int32),
        ("BlasLeafIndices", C.c_void_p), ("BlasLeafIndexCount", C.c_int32),
        ("VertexPositions", C.c_void_p), ("VertexCount", C.c_int32),
        ("Vertices", C.c_void_p),
        ("Meshes", C.c_void_p), ("MeshCount", C.c_int32),
        ("Materials", C.c_void_p), ("MaterialCount", C.c_int32),
        ("MeshTransforms", C.c_void_p), ("MeshTransformCount", C.c_int32),
        ("Lights", C.c_void_p), ("LightCount", C.c_int32),
        ("SkyFaces", C.c_void_p), ("SkyFaceSize", C.c_int32),
        ("Textures", C.c_void_p), ("TextureCount", C.c_int32),
    ]


class Atmosphere(C.Structure):
    """idkpt_atmosphere = AtmosphericScatterer.GpuSettings (Source/Render/AtmosphericScatterer.cs:9-20), same order; the defaults are the reference's."""
    _fields_ = [("ISteps", C.c_int32), ("JSteps", C.c_int32), ("LightIntensity", C.c_float), ("Azimuth", C.c_float), ("Elevation", C.c_float)]

    def __init__(self, ISteps=40, JSteps=8, LightIntensity=15.0, Azimuth=0.0, Elevation=0.0):
        super().__init__(int(ISteps), int(JSteps), float(LightIntensity), float(Azimuth), float(Elevation))


class TonemapSettings(C.Structure):
    """idkpt_tonemap = TonemapAndGammaCorrect.GpuSettings (Source/Render/TonemapAndGammaCorrecter.cs:10-22), same order; the defaults are the reference's."""
    _fields_ = [("Exposure", C.c_float), ("Saturation", C.c_float), ("Linear", C.c_float), ("Peak", C.c_float), ("Compression", C.c_float), ("DoTonemapAndSrgbTransform", C.c_int32)]

    def __init__(self, Exposure=0.45, Saturation=1.06, Linear=0.18, Peak=1.0, Compression=0.1, DoTonemapAndSrgbTransform=True):
        super().__init__(float(Exposure), float(Saturation), float(Linear), float(Peak), float(Compression), 1 if DoTonemapAndSrgbTransform else 0)


IDKPT_DISPLAY_RGBA8, IDKPT_DISPLAY_RGBA32F = 0, 1
IDKPT_BLOOM_ROUTE_TILED, IDKPT_BLOOM_ROUTE_DIRECT = 0, 1   # enum idkpt_bloom_route (idkptGetBloomRoute): how down pass 0 read the image


class BloomSettings(C.Structure):
    """idkpt_bloom = Bloom.GpuSettings (Source/Render/Bloom.cs:10-18) + MinusLods (Bloom.cs:46); the defaults are the reference's."""
    _fields_ = [("Threshold", C.c_float), ("MaxColor", C.c_float), ("MinusLods", C.c_int32)]

    def __init__(self, Threshold=1.5, MaxColor=3.8, MinusLods=3):
        super().__init__(float(Threshold), float(MaxColor), int(MinusLods))


IDKPT_RESULT_NOISY, IDKPT_RESULT_DENOISED = 0, 1           # enum idkpt_result_source (idkptSetResultSource): what image 0 means to idkptPresent and idkptBloom
IDKPT_DENOISE_ROUTE_TILED, IDKPT_DENOISE_ROUTE_DIRECT = 0, 1   # enum idkpt_denoise_route (idkptGetDenoiseRoute): how an iteration reached its taps


class Denoise(C.Structure):
    """idkpt_denoise: the settings of idkptDenoise (include/idkpt.h, "denoised output"; no counterpart in the reference, whose denoiser is OIDN on the host).  The sigma
    defaults are the tuned ones of profiles/denoise.md."""
    _fields_ = [("Iterations", C.c_int32), ("ColorSigma", C.c_float), ("AlbedoSigma", C.c_float), ("NormalSigma", C.c_float), ("DemodulateAlbedo", C.c_int32)]

    def __init__(self, Iterations=5, ColorSigma=8.0, AlbedoSigma=0.2, NormalSigma=0.5, DemodulateAlbedo=True):
        super().__init__(int(Iterations), float(ColorSigma), float(AlbedoSigma), float(NormalSigma), int(DemodulateAlbedo))


class DenoiseVariance(C.Structure):
    """idkpt_denoise_variance: the settings of idkptDenoiseVariance (include/idkpt.h, "variance-guided denoised output"; no counterpart in the reference).  The LumaSigma
    and VarianceEpsilon defaults are the tuned ones of profiles/denoise_variance.md."""
    _fields_ = [("Iterations", C.c_int32), ("LumaSigma", C.c_float), ("VarianceEpsilon", C.c_float), ("AlbedoSigma", C.c_float), ("NormalSigma", C.c_float), ("DemodulateAlbedo", C.c_int32)]

    def __init__(self, Iterations=5, LumaSigma=1.0, VarianceEpsilon=0.1, AlbedoSigma=0.2, NormalSigma=0.5, DemodulateAlbedo=True):
        super().__init__(int(Iterations), float(LumaSigma), float(VarianceEpsilon), float(AlbedoSigma), float(NormalSigma), int(DemodulateAlbedo))


class DenoiseTemporal(C.Structure):
    """idkpt_denoise_temporal: the settings of idkptDenoiseTemporal (include/idkpt.h, "temporal moments"; no counterpart in the reference).  DenoiseVariance's fields and
    SpatialBelow: pixels whose effective sample count is below it take the 7 x 7 spatial estimate of the variance.  The defaults are starting values
    (profiles/denoise_temporal.md)."""
    _fields_ = [("Iterations", C.c_int32), ("LumaSigma", C.c_float), ("VarianceEpsilon", C.c_float), ("AlbedoSigma", C.c_float), ("NormalSigma", C.c_float), ("DemodulateAlbedo", C.c_int32),
                ("SpatialBelow", C.c_float)]

    def __init__(self, Iterations=5, LumaSigma=1.0, VarianceEpsilon=0.1, AlbedoSigma=0.2, NormalSigma=0.5, DemodulateAlbedo=True, SpatialBelow=4.0):
        super().__init__(int(Iterations), float(LumaSigma), float(VarianceEpsilon), float(AlbedoSigma), float(NormalSigma), int(DemodulateAlbedo), float(SpatialBelow))


class Noise(C.Structure):
    """idkpt_noise: the settings of idkptEstimateNoise (include/idkpt.h, "noise estimate"; no counterpart in the reference).  The defaults are starting values nobody has
    tuned (profiles/noise.md)."""
    _fields_ = [("Epsilon", C.c_float), ("Threshold", C.c_float)]

    def __init__(self, Epsilon=1e-2, Threshold=0.05):
        super().__init__(float(Epsilon), float(Threshold))


class NoiseSummary(C.Structure):
    """idkpt_noise_summary: what idkptEstimateNoise leaves beside the tile map"""
    _fields_ = [("TilesAbove", C.c_uint32), ("MaxTileMean", C.c_float), ("Tiles", C.c_uint32), ("Samples", C.c_uint32)]


IDKPT_NO_HISTORY = -2                                                   # idkptReproject's historySlot: start a history
IDKPT_DENOISE_INPUT_ACCUMULATED, IDKPT_DENOISE_INPUT_TEMPORAL = 0, 1    # enum idkpt_denoise_input (idkptSetDenoiseInput): where idkptDenoise takes its colour from


class Reproject(C.Structure):
    """idkpt_reproject: the settings of idkptReproject (include/idkpt.h, "temporal reprojection"; no counterpart in the reference).  PrevProjView / PrevViewPos: the
    ProjView matrix (View * Projection, OpenTK memory order) and the position of the camera the history slot's geometry was captured with.  The PositionTolerance and
    MaxHistory defaults are starting values (profiles/reproject.md)."""
    _fields_ = [("PrevProjView", C.c_float * 16), ("PrevViewPos", C.c_float * 3), ("PositionTolerance", C.c_float), ("MaxHistory", C.c_float)]

    def __init__(self, PrevProjView=None, PrevViewPos=(0.0, 0.0, 0.0), PositionTolerance=0.02, MaxHistory=32.0):
        m = np.eye(4, dtype=np.float32) if PrevProjView is None else np.asarray(PrevProjView, np.float32)
        super().__init__((C.c_float * 16)(*m.reshape(16).tolist()), (C.c_float * 3)(*[float(v) for v in PrevViewPos]), float(PositionTolerance), float(MaxHistory))

    @classmethod
    def from_camera(cls, cam, **kw):
        """the settings for a history frame rendered with scenes.Camera `cam`"""
        return cls((cam.view @ cam.proj).astype(np.float32), cam.position, **kw)


class Rectify(C.Structure):
    """idkpt_rectify: the settings of idkptRectifyHistory (include/idkpt.h, "history rectification"; no counterpart in the reference).  Radius: the window is
    (2 Radius + 1)^2; below ZLow standard errors of disagreement between the fast and the long history nothing happens, from ZHigh on the long history is replaced;
    Epsilon: the absolute noise floor of the difference.  The defaults are starting values (profiles/rectify.md)."""
    _fields_ = [("Radius", C.c_int32), ("ZLow", C.c_float), ("ZHigh", C.c_float), ("Epsilon", C.c_float)]

    def __init__(self, Radius=2, ZLow=3.0, ZHigh=6.0, Epsilon=1e-3):
        super().__init__(int(Radius), float(ZLow), float(ZHigh), float(Epsilon))


class Reconstruct(C.Structure):
    """idkpt_reconstruct: the settings of idkptReconstructHistory (include/idkpt.h, "history reconstruction"; no counterpart in the reference).  Taps at
    p + Stride * (dx, dy), dx and dy in -Radius .. Radius; pixels whose temporal count is below FillBelow are topped up to it from texels of the same surface whose
    count is at least FillBelow; AlbedoSigma / NormalSigma: the guide kernels of the filters.  The defaults are starting values (profiles/reconstruct.md)."""
    _fields_ = [("Radius", C.c_int32), ("Stride", C.c_int32), ("FillBelow", C.c_float), ("AlbedoSigma", C.c_float), ("NormalSigma", C.c_float)]

    def __init__(self, Radius=2, Stride=3, FillBelow=4.0, AlbedoSigma=0.2, NormalSigma=0.5):
        super().__init__(int(Radius), int(Stride), float(FillBelow), float(AlbedoSigma), float(NormalSigma))


class Stats(C.Structure):
    _fields_ = [("RaysTraced", C.c_uint64), ("PrimaryRays", C.c_uint64), ("Frames", C.c_uint64),
                ("LastAliveCounts", C.c_uint32 * 16), ("LastTraceMs", C.c_float), ("LastFrameMs", C.c_float),
                ("NodePairVisits", C.c_uint64), ("TriangleTests", C.c_uint64),
                ("TraceMsTotal", C.c_double), ("TraceLaunches", C.c_uint64),
                ("WideFlaggedRays", C.c_uint64), ("WideNodeVisits", C.c_uint64), ("WideLeafRecords", C.c_uint64), ("WideTriangleTests", C.c_uint64), ("InstTlasFlaggedRays", C.c_uint64),
                ("PacketFlaggedRays", C.c_uint64), ("PacketPackets", C.c_uint64), ("PacketNodeSteps", C.c_uint64), ("PacketLiveLanes", C.c_uint64), ("PacketRaysEntered", C.c_uint64), ("PacketTriangleRounds", C.c_uint64), ("InstUnifiedLaunches", C.c_uint64), ("InstUnifiedEntries", C.c_uint32), ("InstUnifiedTopDepth", C.c_uint32), ("LastOcclusionLaunches", C.c_uint64), ("LastFoldBatches", C.c_uint64)]


def _ptr(a):
    return None if a is None or len(a) == 0 else a.ctypes.data


class Scene:
    """Host-side owner of every array the path tracer consumes (the role of BVH + ModelManager + LightManager
    in the reference).  Arrays are C-contiguous numpy arrays of the dtypes above."""

    def __init__(self):
        self.blas_nodes = np.zeros(0, GpuBlasNode)
        self.blas_triangles = np.zeros(0, GpuBlasTriangle)
        self.blas_descs = np.zeros(0, GpuBlasDesc)
        self.blas_instances = np.zeros(0, GpuBlasInstance)
        self.tlas_nodes = np.zeros(0, GpuTlasNode)
        self.blas_parent_indices = np.zeros(0, np.int32)
        self.blas_leaf_indices = np.zeros(0, np.int32)
        self.vertex_positions = np.zeros((0, 3), np.float32)
        self.vertices = np.zeros(0, GpuVertex)
        self.meshes = np.zeros(0, GpuMesh)
        self.materials = np.zeros(0, GpuMaterial)
        self.mesh_transforms = np.zeros(0, GpuMeshTransform)
        self.lights = np.zeros(0, GpuLight)
        self.sky_faces = None  # (6, S, S, 4) float32
        self.textures = []     # list of (h, w, 4) float32 arrays (REPEAT, LINEAR) or TextureImage objects (sampler state, 8-bit formats)
        self.blas_stack_size = 0

    def desc(self):
        """Returns (SceneDesc, keepalive) — keepalive must outlive the call that consumes the desc."""
        keep = []

        def c(a, dt=None):
            a = np.ascontiguousarray(a, dtype=dt)
            keep.append(a)
            return a

        d = SceneDesc()
        a = c(self.blas_nodes); d.BlasNodes, d.BlasNodeCount = _ptr(a), len(a)
        a = c(self.blas_triangles); d.BlasTriangles, d.BlasTriangleCount = _ptr(a), len(a)
        a = c(self.blas_descs); d.BlasDescs, d.BlasDescCount = _ptr(a), len(a)
        a = c(self.blas_instances); d.BlasInstances, d.BlasInstanceCount = _ptr(a), len(a)
        a = c(self.tlas_nodes); d.TlasNodes, d.TlasNodeCount = _ptr(a), len(a)
        a = c(self.blas_parent_indices, np.int32); d.BlasParentIndices, d.BlasParentIndexCount = _ptr(a), len(a)
        a = c(self.blas_leaf_indices, np.int32); d.BlasLeafIndices, d.BlasLeafIndexCount = _ptr(a), len(a)
        a = c(self.vertex_positions, np.float32); d.VertexPositions, d.VertexCount = _ptr(a), len(a)
        a = c(self.vertices); d.Vertices = _ptr(a)
        assert len(a) == d.VertexCount
        a = c(self.meshes); d.Meshes, d.MeshCount = _ptr(a), len(a)
        a = c(self.materials); d.Materials, d.MaterialCount = _ptr(a), len(a)
        a = c(self.mesh_transforms); d.MeshTransforms, d.MeshTransformCount = _ptr(a), len(a)
        a = c(self.lights); d.Lights, d.LightCount = _ptr(a), len(a)
        if self.sky_faces is not None:
            a = c(self.sky_faces, np.float32)
            assert a.ndim == 4 and a.shape[0] == 6 and a.shape[1] == a.shape[2] and a.shape[3] == 4
            d.SkyFaces, d.SkyFaceSize = a.ctypes.data, a.shape[1]
        if self.textures:
            arr = (Texture * len(self.textures))()
            for i, t in enumerate(self.textures):
                t = TextureImage.of(t); keep.append(t)
                t.fill(arr[i])
            keep.append(arr)
            d.Textures, d.TextureCount = C.addressof(arr), len(self.textures)
        return d, keep

# enum idkpt_buffer (include/idkpt.h)
(IDKPT_BUF_MESH_TRANSFORMS, IDKPT_BUF_VERTEX_POSITIONS, IDKPT_BUF_VERTICES, IDKPT_BUF_MESHES, IDKPT_BUF_MATERIALS, IDKPT_BUF_LIGHTS,
 IDKPT_BUF_BLAS_NODES, IDKPT_BUF_TLAS_NODES, IDKPT_BUF_JOINT_MATRICES, IDKPT_BUF_WIDE_NODES, IDKPT_BUF_WIDE_LEAVES, IDKPT_BUF_WIDE_COUNTS, IDKPT_BUF_PREV_VERTEX_POSITIONS,
 IDKPT_BUF_MOTION_PREV_POSITIONS) = range(14)

# GpuPerFrameData (include/idkpt_types.h; Source/GpuTypes/GpuPerFrameData.cs:5-21): the path tracer reads InvView, ViewPos and InvProjection
GpuPerFrameData = np.dtype([("ProjView", "<f4", 16), ("View", "<f4", 16), ("InvView", "<f4", 16), ("PrevView", "<f4", 16), ("ViewPos", "<f4", 3), ("Frame", "<u4"),
                            ("Projection", "<f4", 16), ("InvProjection", "<f4", 16), ("InvProjView", "<f4", 16), ("PrevProjView", "<f4", 16),
                            ("NearPlane", "<f4"), ("FarPlane", "<f4"), ("DeltaRenderTime", "<f4"), ("Time", "<f4")])
assert GpuPerFrameData.itemsize == 544 and GpuPerFrameData.fields["InvView"][1] == 128 and GpuPerFrameData.fields["ViewPos"][1] == 256 and GpuPerFrameData.fields["InvProjection"][1] == 336


# ray queries / RT shadows (include/idkpt.h: idkpt_ray, idkpt_hit, idkpt_shadow_params, enum idkpt_trace_flags)
RayQuery = np.dtype([("Origin", "<f4", 3), ("MaxDist", "<f4"), ("Direction", "<f4", 3), ("_pad0", "<u4")])
RayHit = np.dtype([("T", "<f4"), ("BaryX", "<f4"), ("BaryY", "<f4"), ("TriangleId", "<u4"), ("MeshTransformId", "<u4"), ("Hit", "<u4"),
                   ("_pad0", "<u4"), ("_pad1", "<u4")])
assert RayQuery.itemsize == 32 and RayHit.itemsize == 32
IDKPT_TRACE_ANY_HIT, IDKPT_TRACE_LIGHTS = 1, 2


# sphere collision queries (include/idkpt.h: idkpt_collide_settings, idkpt_moving_sphere, idkpt_sphere_collision, enum idkpt_collide_response)
IDKPT_COLLIDE_NONE, IDKPT_COLLIDE_SLIDE, IDKPT_COLLIDE_REFLECT = 0, 1, 2
MovingSphere = np.dtype([("PrevPosition", "<f4", 3), ("Radius", "<f4"), ("Position", "<f4", 3), ("_pad0", "<u4"), ("Velocity", "<f4", 3), ("_pad1", "<u4")])
SphereCollision = np.dtype([("Position", "<f4", 3), ("HitCount", "<u4"), ("Velocity", "<f4", 3), ("TriangleId", "<u4"), ("Center", "<f4", 3), ("BlasInstanceId", "<u4"),
                            ("SlidingNormal", "<f4", 3), ("PenetrationDepth", "<f4"), ("TriNormal", "<f4", 3), ("Distance", "<f4"), ("TriCollidingPoint", "<f4", 3), ("_pad", "<u4")])
assert MovingSphere.itemsize == 48 and SphereCollision.itemsize == 96


class CollideSettings(C.Structure):
    _fields_ = [("TestSteps", C.c_int32), ("RecursiveSteps", C.c_int32), ("EpsilonNormalOffset", C.c_float), ("Response", C.c_int32), ("UseTlas", C.c_int32), ("_pad", C.c_int32 * 3)]


assert C.sizeof(CollideSettings) == 32


class ShadowParams(C.Structure):
    _fields_ = [("InvProjView", C.c_float * 16), ("TaaJitter", C.c_float * 2), ("Width", C.c_int32), ("Height", C.c_int32),
                ("LightIndex", C.c_int32), ("RayTracingSamples", C.c_int32), ("NoiseIndex", C.c_uint32), ("_pad0", C.c_uint32)]

    @staticmethod
    def make(inv_proj_view, width, height, light_index, samples=1, noise_index=0, jitter=(0.0, 0.0)):
        p = ShadowParams()
        m = np.ascontiguousarray(inv_proj_view, np.float32).reshape(16)
        for i in range(16):
            p.InvProjView[i] = float(m[i])
        p.TaaJitter[0], p.TaaJitter[1] = float(jitter[0]), float(jitter[1])
        p.Width, p.Height, p.LightIndex, p.RayTracingSamples, p.NoiseIndex = width, height, light_index, samples, noise_index
        return p
