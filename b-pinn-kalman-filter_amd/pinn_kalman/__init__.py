"""PINN path of the reference (pinn_kalman/): FlowNet + PressureNet and the
Navier-Stokes residual, on the gfx950 correlation / grid_sample kernels; the Kalman side on
the ns_step simulator: the patch UKF (`ukf`), strong-constraint 4D-Var (`fourdvar`) and the
local ensemble transform Kalman filter (`enkf`)."""
