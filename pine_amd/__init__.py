"""pine_amd -- MI355X-native PathIntegrator, AOIntegrator, DenoiseIntegrator, Accel ray-query and Shader vertex-query hot paths of wicstas/pine."""
from .api import (  # noqa: F401
    Scene, Diffuse, Emissive, Uber, Subsurface, Metal, Glossy, Glass, Node, Position, Normal, UV, Checkerboard, Vec3, lerp,
    node_abs, node_sqr, node_sqrt, node_fract, Image, Texture, Texturef, Noisef, Noise3f, PointLight, SpotLight, DirectionalLight, Sky, ImageSky, Atmosphere, Rect, AABB, OBB, Box, Sphere, Disk, Cone, Mesh, Plane, Line, Cylinder, Triangle,
    Film, Uncharted2, ACES, ThinLenCamera, BlueSampler, SobolSampler, HaltonSampler, PathIntegrator, AOIntegrator, DenoiseIntegrator, guides, denoise, Plan, PineError, Accel, AccelHits, HIT_DTYPE,
    Shader, ShaderRecords, WavefrontPathIntegrator, RECORD_DTYPE,
    mat4, translate, scale, rotate_x, rotate_y, rotate_z, inverse, look_at, film_unpack, packed_offset,
)
