"""DPS deblurring on the NetCDF DDPM: nc_ddpmpp_inpaint_dps with the operator section
replaced by the Gaussian blur operator (13 taps per axis, variance 4; inverse/operators.py
GaussianBlurOperator).  Observation variance and solver as in the inpainting config."""
from configs._configdict import ConfigDict
from configs.vp import nc_ddpmpp


def get_config():
    c = nc_ddpmpp.get_config()
    c.training.batch_size = 16
    c.inverse = ConfigDict(dict(operator="gaussian_blur", blur_size=13, blur_std=4.0, sampler="dps",
                                variance=0.1, solver="RK45"))
    return c
