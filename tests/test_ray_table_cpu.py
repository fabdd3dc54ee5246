"""CPU half of tests/test_ray_table_gpu.py: the new hooks refuse bad arguments before they ask for a device, and the helper's
cameras are what the GPU cases take them for."""
import ctypes as C

import numpy as np

import ray_table_cases as RC

E_ARG = -3   # include/volpath.h VP_E_ARG


def _err(vp):
    return vp.lib().vp_last_error().decode()


def test_camera_ray_hook_validates_its_arguments():
    import volpath as vp
    L = vp.lib()
    px = np.array([0 | (0 << 16), 23 | (15 << 16)], np.uint32)
    out = np.zeros((2, 6), np.float32)
    p, o = px.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    assert L.vp_test_camera_ray(24, 16, p, o, -1) == E_ARG and "negative" in _err(vp)
    assert L.vp_test_camera_ray(24, 16, None, o, 2) == E_ARG
    assert L.vp_test_camera_ray(24, 16, p, None, 2) == E_ARG
    assert L.vp_test_camera_ray(0, 16, p, o, 2) == E_ARG
    assert L.vp_test_camera_ray(24, 65537, p, o, 2) == E_ARG
    assert L.vp_test_camera_ray(23, 16, p, o, 2) == E_ARG and "outside" in _err(vp)      # x = 23 of a 23-wide image
    assert L.vp_test_camera_ray(24, 15, p, o, 2) == E_ARG and "outside" in _err(vp)
    assert not out.any()


def test_ray_table_hook_validates_its_arguments():
    import volpath as vp
    L = vp.lib()
    P = vp.make_param(24, 16)
    out = np.zeros(8, np.float32)
    assert L.vp_get_ray_table(None, out.ctypes.data_as(C.c_void_p), 8) == E_ARG
    assert L.vp_get_ray_table(C.byref(P), None, 8) == E_ARG
    assert L.vp_last_ray_table() == 0


def test_cameras_of_the_cases():
    import volpath as vp
    cams = RC.cameras(vp)
    assert set(cams) == {"default", "orbit0", "orbit1", "orbit2", "orbit3", "inside", "axis", "partial"}
    for name, m in cams.items():
        R = np.array(m, np.float64).reshape(3, 4)[:, :3]
        assert np.allclose(R.T @ R, np.eye(3), atol=1e-6), name
    assert cams["axis"] == (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 3.0)
    eye = np.array(cams["inside"]).reshape(3, 4)[:, 3]
    assert (np.abs(eye) < 1.0).all(), "the camera is not inside the box of a cubic volume"
