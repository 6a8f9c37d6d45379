"""The factor level of bundle adjustment -- proj_eval, imu_ctx / imu_raw_col (csrc/ba_factors.h), prior_pass and the sqrt-info
prologue imu_sqrt_info / imu_sqrt_info_ref (csrc/ba_pipeline.hip), through Handle.ba_eval_factors -- against an 80-bit restatement of
IMUFactor / ProjectionFactor / ProjectionTdFactor / MarginalizationFactor::Evaluate, every block in its own scale
(tests/factor_ref.py: reference, metric, case table, yardstick, edits).

The older factor checks hold an IMU row to 1e-6 of its row weight sum|W_row|: a tenth of the structurally non-zero entries of the
weighted IMU Jacobians are smaller than that and could hold anything.  Here the weighted output is multiplied by the 80-bit U
(covariance = U U^T) and the factor's raw 3 x 3 blocks, which come back, are measured each against its own largest entry.

The bound.  e64(case) = the error of the float64 restatement (bit for bit oracle/ba_numpy) against the 80-bit one; E64 = its largest
value over the case table, one per field kind; the device must stay within M[kind] * E64[kind].  M is the smallest power of two that
the worst measured ratio of emulator and MI355X stays under with a factor 2 to spare (MEASURED).  Every edit of
test_each_edit_exceeds_twice_the_bound must produce more than 2 * M * E64 in some case and kind.

The emulated half (`not gpu`) runs everything the GPU half runs: nothing is cut."""
import numpy as np
import pytest

from oracle import ba_numpy as B
from vins_mono_amd import ba

import factor_ref as R

M = R.M
MEASURED = """E64 (no device involved) and the case that sets it:
    imu_J 5.05e-14 (n99_dt0.1/perturbed/bias_far/antipodal: |U||W| = 1.2e3 on the 9.9 s record), imu_r 3.16e-14 (n2/consistent/bias1e-4/plain:
    3 m positions whose difference is 5e-4 m), imu_J_far = imu_r_far 2.66e-9 (n2/consistent/bias1e-4/far_position: 1e5 m for 5e-4 m),
    proj_J 2.92e-14 (plain), proj_J_lambda 1.58e-9 (plain: lambda = 1e-4 across the zero baseline, the block is 1.2e-7 of its terms),
    proj_r 9.28e-15 (ex), prior_r 4.22e-14 (old_K11_n75/dx1e-3), prior_r_x0 1.54e-11 (old_K11_n75/at_x0)
M, the smallest power of two above twice the worst ratio below: imu_J 2, imu_r 4, imu_J_far 4, imu_r_far 4, the four in the
    reference-info mode 4 each (its imu_J reaches 1.60 on the 9.9 s record: inverse() then LLT, as the float64 route), proj_J 2, proj_J_lambda 8,
    proj_r 4, prior_r 2, prior_r_x0 1.  The ratios of 1.00 are cases in which device and oracle lose the same thing: the rounding of
    0.5 g dt^2 + P_j - P_i, which both form in the reference's order.
IMU cases, record_error / E64: J r in the default info mode, J r in the reference-info mode (far_position rows: the *_far kinds)
                                                 CPU fiber emulator       MI355X
    n2/consistent/bias0/plain                     0.46  0.73  0.45  0.73     0.48  0.78  0.49  0.78
    n2/consistent/bias1e-4/plain                  0.63  1.00  0.63  1.00     0.62  1.00  0.62  1.00
    n2/consistent/bias_far/plain                  0.46  0.74  0.46  0.74     0.48  0.77  0.48  0.77
    n2/perturbed/bias0/plain                      0.01  0.01  0.02  0.02     0.01  0.01  0.01  0.02
    n2/perturbed/bias1e-4/plain                   0.01  0.02  0.01  0.02     0.01  0.02  0.01  0.02
    n2/perturbed/bias_far/plain                   0.01  0.01  0.01  0.01     0.01  0.02  0.01  0.02
    n2/consistent/bias1e-4/antipodal              0.41  0.67  0.41  0.67     0.41  0.67  0.41  0.67
    n2/perturbed/bias_far/antipodal               0.01  0.01  0.01  0.01     0.01  0.01  0.01  0.01
    n2/consistent/bias1e-4/rot178                 0.55  0.89  0.55  0.89     0.55  0.88  0.55  0.88
    n2/perturbed/bias_far/rot178                  0.01  0.01  0.02  0.01     0.01  0.02  0.02  0.01
    n2/consistent/bias1e-4/far_position           1.00  1.00  1.00  1.00     1.00  1.00  1.00  1.00
    n2/perturbed/bias_far/far_position            0.00  0.00  0.00  0.00     0.00  0.00  0.00  0.00
    n20/consistent/bias0/plain                    0.04  0.06  0.05  0.06     0.04  0.05  0.06  0.05
    n20/consistent/bias1e-4/plain                 0.04  0.06  0.05  0.06     0.04  0.06  0.05  0.06
    n20/consistent/bias_far/plain                 0.04  0.06  0.05  0.06     0.03  0.05  0.05  0.05
    n20/perturbed/bias0/plain                     0.02  0.03  0.05  0.03     0.02  0.02  0.05  0.03
    n20/perturbed/bias1e-4/plain                  0.02  0.02  0.05  0.04     0.02  0.02  0.05  0.03
    n20/perturbed/bias_far/plain                  0.02  0.03  0.05  0.02     0.02  0.03  0.06  0.02
    n20/consistent/bias1e-4/antipodal             0.04  0.05  0.08  0.05     0.03  0.05  0.09  0.05
    n20/perturbed/bias_far/antipodal              0.04  0.03  0.09  0.03     0.04  0.03  0.09  0.03
    n20/consistent/bias1e-4/rot178                0.03  0.05  0.07  0.05     0.03  0.05  0.07  0.05
    n20/perturbed/bias_far/rot178                 0.02  0.01  0.07  0.04     0.02  0.01  0.07  0.04
    n20/consistent/bias1e-4/far_position          0.00  0.00  0.00  0.00     0.00  0.00  0.00  0.00
    n20/perturbed/bias_far/far_position           0.00  0.00  0.00  0.00     0.00  0.00  0.00  0.00
    n64/consistent/bias0/plain                    0.02  0.00  0.09  0.00     0.02  0.00  0.09  0.00
    n64/consistent/bias1e-4/plain                 0.02  0.00  0.09  0.00     0.02  0.01  0.09  0.01
    n64/consistent/bias_far/plain                 0.02  0.01  0.09  0.01     0.02  0.01  0.09  0.01
    n64/perturbed/bias0/plain                     0.02  0.02  0.10  0.06     0.02  0.02  0.10  0.07
    n64/perturbed/bias1e-4/plain                  0.02  0.01  0.09  0.02     0.02  0.00  0.09  0.02
    n64/perturbed/bias_far/plain                  0.01  0.01  0.09  0.09     0.01  0.01  0.09  0.09
    n64/consistent/bias1e-4/antipodal             0.01  0.01  0.11  0.01     0.01  0.01  0.11  0.01
    n64/perturbed/bias_far/antipodal              0.01  0.01  0.11  0.02     0.01  0.01  0.11  0.02
    n64/consistent/bias1e-4/rot178                0.01  0.01  0.09  0.02     0.01  0.01  0.09  0.01
    n64/perturbed/bias_far/rot178                 0.04  0.02  0.62  0.05     0.05  0.02  0.62  0.06
    n64/consistent/bias1e-4/far_position          0.00  0.00  0.00  0.00     0.00  0.00  0.00  0.00
    n64/perturbed/bias_far/far_position           0.00  0.00  0.00  0.00     0.00  0.00  0.00  0.00
    varying_dt/consistent/bias0/plain             0.01  0.01  0.04  0.01     0.01  0.01  0.04  0.01
    varying_dt/consistent/bias1e-4/plain          0.03  0.04  0.05  0.04     0.03  0.04  0.05  0.04
    varying_dt/consistent/bias_far/plain          0.02  0.04  0.05  0.04     0.02  0.04  0.04  0.04
    varying_dt/perturbed/bias0/plain              0.01  0.02  0.04  0.02     0.01  0.02  0.05  0.02
    varying_dt/perturbed/bias1e-4/plain           0.01  0.02  0.04  0.04     0.02  0.03  0.04  0.06
    varying_dt/perturbed/bias_far/plain           0.01  0.01  0.04  0.02     0.01  0.01  0.05  0.02
    varying_dt/consistent/bias1e-4/antipodal      0.03  0.00  0.04  0.00     0.03  0.01  0.04  0.01
    varying_dt/perturbed/bias_far/antipodal       0.03  0.02  0.03  0.04     0.03  0.03  0.03  0.01
    varying_dt/consistent/bias1e-4/rot178         0.01  0.03  0.04  0.02     0.01  0.02  0.03  0.02
    varying_dt/perturbed/bias_far/rot178          0.01  0.01  0.03  0.05     0.01  0.01  0.04  0.05
    varying_dt/consistent/bias1e-4/far_position   0.00  0.00  0.00  0.00     0.00  0.00  0.00  0.00
    varying_dt/perturbed/bias_far/far_position    0.00  0.00  0.00  0.00     0.00  0.00  0.00  0.00
    fast_rotation/consistent/bias0/plain          0.02  0.03  0.08  0.03     0.02  0.02  0.08  0.02
    fast_rotation/consistent/bias1e-4/plain       0.02  0.01  0.08  0.01     0.02  0.01  0.08  0.01
    fast_rotation/consistent/bias_far/plain       0.02  0.02  0.08  0.02     0.02  0.02  0.08  0.02
    fast_rotation/perturbed/bias0/plain           0.03  0.02  0.08  0.05     0.02  0.03  0.08  0.05
    fast_rotation/perturbed/bias1e-4/plain        0.02  0.01  0.08  0.02     0.03  0.02  0.08  0.02
    fast_rotation/perturbed/bias_far/plain        0.02  0.04  0.08  0.04     0.02  0.04  0.08  0.04
    fast_rotation/consistent/bias1e-4/antipodal   0.05  0.02  0.15  0.02     0.05  0.02  0.14  0.02
    fast_rotation/perturbed/bias_far/antipodal    0.05  0.04  0.14  0.03     0.05  0.01  0.15  0.03
    fast_rotation/consistent/bias1e-4/rot178      0.03  0.02  0.11  0.03     0.03  0.03  0.12  0.03
    fast_rotation/perturbed/bias_far/rot178       0.04  0.05  0.10  0.05     0.03  0.05  0.11  0.05
    fast_rotation/consistent/bias1e-4/far_position  0.00  0.00  0.00  0.00     0.00  0.00  0.00  0.00
    fast_rotation/perturbed/bias_far/far_position  0.00  0.00  0.00  0.00     0.00  0.00  0.00  0.00
    n99_dt0.1/consistent/bias0/plain              0.02  0.00  1.53  0.00     0.02  0.00  1.53  0.00
    n99_dt0.1/consistent/bias1e-4/plain           0.02  0.01  1.59  0.01     0.02  0.01  1.59  0.01
    n99_dt0.1/consistent/bias_far/plain           0.01  0.00  1.56  0.00     0.01  0.00  1.56  0.00
    n99_dt0.1/perturbed/bias0/plain               0.02  0.01  1.53  0.03     0.02  0.01  1.53  0.03
    n99_dt0.1/perturbed/bias1e-4/plain            0.02  0.01  1.60  0.01     0.02  0.00  1.60  0.01
    n99_dt0.1/perturbed/bias_far/plain            0.02  0.01  1.53  0.01     0.02  0.01  1.53  0.01
    n99_dt0.1/consistent/bias1e-4/antipodal       0.02  0.01  1.28  0.01     0.03  0.01  1.28  0.01
    n99_dt0.1/perturbed/bias_far/antipodal        0.03  0.01  1.28  0.01     0.02  0.01  1.28  0.01
    n99_dt0.1/consistent/bias1e-4/rot178          0.02  0.01  1.58  0.04     0.02  0.01  1.58  0.05
    n99_dt0.1/perturbed/bias_far/rot178           0.02  0.01  1.29  0.02     0.02  0.01  1.29  0.02
    n99_dt0.1/consistent/bias1e-4/far_position    0.00  0.00  0.00  0.00     0.00  0.00  0.00  0.00
    n99_dt0.1/perturbed/bias_far/far_position     0.00  0.00  0.00  0.00     0.00  0.00  0.00  0.00
    n120_dt0.1/perturbed/bias1e-4/plain          skipped (sum_dt = 12 s): rows exactly zero in both modes, on both
projection factors, J r (lam: the lambda block where it is of the proj_J_lambda kind); 0-1 is the zero baseline, 0-2 the forward motion
    plain/lambda1e-4/0-1                          0.08  0.02  2.79     0.08  0.03  3.66
    plain/lambda1e-4/0-2                          0.12  0.06  0.05     0.26  0.04  0.04
    plain/lambda1e-3/0-1                          0.09  0.07  0.45     0.09  0.06  0.34
    plain/lambda1e-3/0-2                          0.11  0.03  0.00     0.13  0.01  0.00
    plain/lambda0.2/0-1                           0.09  0.08  0.01     0.08  0.07  0.00
    plain/lambda0.2/0-2                           0.41  0.10   -       0.07  0.02   -  
    plain/lambda20/0-1                            0.16  1.02  0.00     0.18  1.02  0.00
    plain/image_edge/0-1                          0.11  0.09  0.02     0.08  0.03  0.01
    plain/image_edge/0-2                          0.10  0.05   -       0.14  0.02   -  
    plain/z_j0.1/0-1                              0.09  0.08  0.00     0.16  0.08  0.00
    plain/z_j0.1/0-2                              0.11  0.09  0.00     0.11  0.13  0.00
    plain/td_plus_minus/0-1                       0.07  0.03  0.00     0.08  0.03  0.00
    plain/td_plus_minus/0-2                       0.17  0.02   -       0.27  0.02   -  
    plain/td_minus_plus/0-1                       0.16  0.06  0.00     0.09  0.04  0.01
    plain/td_minus_plus/0-2                       0.20  0.03   -       0.30  0.02   -  
    plain/row_top/0-1                             0.18  0.05  0.00     0.08  0.05  0.00
    plain/row_top/0-2                             0.14  0.05   -       0.11  0.05   -  
    plain/row_bottom/0-1                          0.10  0.05  0.01     0.09  0.05  0.01
    plain/row_bottom/0-2                          0.09  0.03   -       0.11  0.03   -  
    plain/velocity0/0-1                           0.10  0.04  0.00     0.08  0.04  0.00
    plain/velocity0/0-2                           0.07  0.01   -       0.07  0.02   -  
    ex/lambda1e-4/0-1                             0.08  0.01  0.55     0.08  0.01  0.69
    ex/lambda1e-4/0-2                             0.13  0.05  0.03     0.16  0.06  0.03
    ex/lambda1e-3/0-1                             0.12  0.02  0.03     0.08  0.02  0.10
    ex/lambda1e-3/0-2                             0.12  0.02  0.00     0.12  0.02  0.00
    ex/lambda0.2/0-1                              0.08  0.03  0.00     0.09  0.05  0.00
    ex/lambda0.2/0-2                              0.09  0.03   -       0.13  0.03   -  
    ex/lambda20/0-1                               0.11  1.00  0.00     0.09  1.09  0.00
    ex/image_edge/0-1                             0.11  0.07  0.01     0.09  0.03  0.00
    ex/image_edge/0-2                             0.20  0.03   -       0.14  0.02   -  
    ex/z_j0.1/0-1                                 0.10  0.06  0.00     0.12  0.06  0.00
    ex/z_j0.1/0-2                                 0.08  0.20  0.00     0.08  0.20  0.00
    ex/td_plus_minus/0-1                          0.08  0.05  0.00     0.08  0.02  0.00
    ex/td_plus_minus/0-2                          0.35  0.06   -       0.19  0.05   -  
    ex/td_minus_plus/0-1                          0.17  0.05  0.00     0.08  0.04  0.00
    ex/td_minus_plus/0-2                          0.20  0.03   -       0.33  0.01   -  
    ex/row_top/0-1                                0.10  0.03  0.00     0.10  0.06  0.00
    ex/row_top/0-2                                0.09  0.03   -       0.07  0.03   -  
    ex/row_bottom/0-1                             0.10  0.02  0.00     0.10  0.05  0.00
    ex/row_bottom/0-2                             0.12  0.01   -       0.21  0.01   -  
    ex/velocity0/0-1                              0.10  0.03  0.00     0.09  0.04  0.00
    ex/velocity0/0-2                              0.07  0.03   -       0.07  0.02   -  
    td/lambda1e-4/0-1                             0.08  0.02  2.80     0.08  0.03  3.66
    td/lambda1e-4/0-2                             0.12  0.06  0.05     0.26  0.04  0.04
    td/lambda1e-3/0-1                             0.09  0.07  0.45     0.09  0.06  0.34
    td/lambda1e-3/0-2                             0.11  0.03  0.00     0.19  0.01  0.00
    td/lambda0.2/0-1                              0.09  0.08  0.01     0.08  0.07  0.00
    td/lambda0.2/0-2                              0.41  0.10   -       0.16  0.02   -  
    td/lambda20/0-1                               0.16  1.02  0.00     0.18  1.02  0.00
    td/image_edge/0-1                             0.11  0.09  0.02     0.08  0.03  0.01
    td/image_edge/0-2                             0.10  0.05   -       0.14  0.02   -  
    td/z_j0.1/0-1                                 0.09  0.08  0.00     0.16  0.08  0.00
    td/z_j0.1/0-2                                 0.11  0.09  0.00     0.11  0.13  0.00
    td/td_plus_minus/0-1                          0.07  0.04  0.00     0.09  0.02  0.00
    td/td_plus_minus/0-2                          0.13  0.03   -       0.18  0.02   -  
    td/td_minus_plus/0-1                          0.14  0.03  0.00     0.08  0.04  0.00
    td/td_minus_plus/0-2                          0.24  0.04   -       0.21  0.03   -  
    td/row_top/0-1                                0.18  0.05  0.00     0.08  0.05  0.00
    td/row_top/0-2                                0.14  0.05   -       0.11  0.05   -  
    td/row_bottom/0-1                             0.10  0.05  0.01     0.09  0.05  0.01
    td/row_bottom/0-2                             0.09  0.03   -       0.11  0.03   -  
    td/velocity0/0-1                              0.10  0.04  0.00     0.08  0.04  0.00
    td/velocity0/0-2                              0.07  0.01   -       0.07  0.02   -  
    ex_td_tr/lambda1e-4/0-1                       0.08  0.02  0.72     0.08  0.02  0.73
    ex_td_tr/lambda1e-4/0-2                       0.11  0.11  0.08     0.14  0.03  0.06
    ex_td_tr/lambda1e-3/0-1                       0.12  0.07  0.10     0.09  0.07  0.06
    ex_td_tr/lambda1e-3/0-2                       0.29  0.02  0.00     0.11  0.04  0.00
    ex_td_tr/lambda0.2/0-1                        0.09  0.08  0.00     0.09  0.07  0.00
    ex_td_tr/lambda0.2/0-2                        0.26  0.09   -       0.14  0.03   -  
    ex_td_tr/lambda20/0-1                         0.14  0.40  0.00     0.08  0.39  0.00
    ex_td_tr/image_edge/0-1                       0.12  0.08  0.01     0.11  0.08  0.01
    ex_td_tr/image_edge/0-2                       0.13  0.03   -       0.11  0.02   -  
    ex_td_tr/z_j0.1/0-1                           0.11  0.03  0.00     0.08  0.03  0.00
    ex_td_tr/z_j0.1/0-2                           0.05  0.08  0.00     0.06  0.09  0.00
    ex_td_tr/td_plus_minus/0-1                    0.09  0.03  0.00     0.08  0.02  0.00
    ex_td_tr/td_plus_minus/0-2                    0.36  0.02   -       0.11  0.03   -  
    ex_td_tr/td_minus_plus/0-1                    0.14  0.09  0.00     0.09  0.08  0.00
    ex_td_tr/td_minus_plus/0-2                    0.27  0.03   -       0.39  0.05   -  
    ex_td_tr/row_top/0-1                          0.09  0.05  0.00     0.10  0.04  0.00
    ex_td_tr/row_top/0-2                          0.10  0.04   -       0.09  0.04   -  
    ex_td_tr/row_bottom/0-1                       0.14  0.03  0.00     0.09  0.04  0.00
    ex_td_tr/row_bottom/0-2                       0.11  0.02   -       0.12  0.02   -  
    ex_td_tr/velocity0/0-1                        0.10  0.03  0.00     0.09  0.04  0.00
    ex_td_tr/velocity0/0-2                        0.07  0.03   -       0.07  0.02   -  
    relo: worst of the 170 window factors         0.53  0.76  0.00     0.61  1.15  0.00
    relo: worst of the 8 relocalisation factors   0.21  0.22  0.00     0.10  0.09  0.00
prior cases, prior_r (at_x0 rows but the dyadic one: prior_r_x0)
    old_K4/at_x0                                  0.02     0.01
    old_K4/dx1e-3                                 0.16     0.35
    old_K4/dx0.3                                  0.00     0.01
    old_K4/antipodal                              0.26     0.30
    old_K4/rot179                                 0.01     0.02
    old_K4_ex_td/at_x0                            0.00     0.00
    old_K4_ex_td/dx1e-3                           0.41     0.63
    old_K4_ex_td/dx0.3                            0.01     0.00
    old_K4_ex_td/antipodal                        0.22     0.49
    old_K4_ex_td/rot179                           0.01     0.01
    second_new_K4/at_x0                           0.00     0.00
    second_new_K4/dx1e-3                          0.18     0.14
    second_new_K4/dx0.3                           0.00     0.00
    second_new_K4/antipodal                       0.16     0.11
    second_new_K4/rot179                          0.01     0.01
    old_K11_n75/at_x0                             0.06     0.42
    old_K11_n75/dx1e-3                            0.48     0.55
    old_K11_n75/dx0.3                             0.00     0.00
    old_K11_n75/antipodal                         0.81     0.48
    old_K11_n75/rot179                            0.02     0.01
    dyadic/at_x0                                  0.00     0.00
    dyadic/dx1e-3                                 0.00     0.00
    dyadic/dx0.3                                  0.00     0.00
    dyadic/antipodal                              0.15     0.15
    dyadic/rot179                                 0.00     0.01
worst ratio per kind (emulator | MI355X) and the M it gives
    imu_J                0.63 n2/consistent/bias1e-4/plain | 0.62 n2/consistent/bias1e-4/plain
    imu_r                1.00 n2/consistent/bias1e-4/plain | 1.00 n2/consistent/bias1e-4/plain
    imu_J_far            1.00 n2/consistent/bias1e-4/far_position | 1.00 n2/consistent/bias1e-4/far_position
    imu_r_far            1.00 n2/consistent/bias1e-4/far_position | 1.00 n2/consistent/bias1e-4/far_position
    imu_J_refinfo        1.60 n99_dt0.1/perturbed/bias1e-4/plain | 1.60 n99_dt0.1/perturbed/bias1e-4/plain
    imu_r_refinfo        1.00 n2/consistent/bias1e-4/plain | 1.00 n2/consistent/bias1e-4/plain
    imu_J_far_refinfo    1.00 n2/consistent/bias1e-4/far_position | 1.00 n2/consistent/bias1e-4/far_position
    imu_r_far_refinfo    1.00 n2/consistent/bias1e-4/far_position | 1.00 n2/consistent/bias1e-4/far_position
    proj_J               0.53 relo/f130 | 0.61 relo/f136
    proj_r               1.02 td/lambda20/0-1 | 1.15 relo/f136
    proj_J_lambda        2.80 td/lambda1e-4/0-1 | 3.66 td/lambda1e-4/0-1
    prior_r_x0           0.06 old_K11_n75/at_x0 | 0.42 old_K11_n75/at_x0
    prior_r              0.81 old_K11_n75/antipodal | 0.63 old_K4_ex_td/dx1e-3
mutation condition, largest error of the edited float64 restatement over the table (the case); the kind's 2 * M * E64 = imu_J 4.0e-13 (M of
the reference-info mode), imu_r 2.5e-13, proj_J 1.2e-13, proj_J_lambda 2.5e-8, proj_r 7.4e-14, prior_r 1.7e-13:
    imu_dtheta_i_delta_q           imu_J 4.9e-1 (n99_dt0.1/perturbed/bias_far/antipodal)
    imu_dbg_i_corrected_delta_q    imu_J 5.6e-1 (n99_dt0.1/perturbed/bias_far/rot178)
    imu_r_without_dq_dbg           imu_r 4.4e-1 (n99_dt0.1/perturbed/bias_far/plain)
    imu_r_without_dp_dbg           imu_r 3.2e-1 (n99_dt0.1/consistent/bias_far/plain)
    imu_dtheta_j_qright            imu_J 2.0 (n64/consistent/bias1e-4/rot178)
    imu_r_w_flip                   imu_r 1.7 (varying_dt/perturbed/bias_far/rot178)
    imu_W_p_bg_entry               imu_J 2.8e-12 (n99_dt0.1/perturbed/bias_far/rot178): W[1][13] x (1 + 1e-9), 7 x the bound
    proj_row_term_dropped          proj_J 8.1e-2, proj_r 6.3e-2 (ex_td_tr)
    proj_cur_td_of_j_for_i         proj_J 1.5, proj_r 5.0e-1 (td)
    proj_td_without_vel_j          proj_J 24 (td)
    proj_lambda_one_over_lambda    proj_J 9.1e-1 (relo), proj_J_lambda 19 (ex_td_tr)
    proj_ex_third_skew_dropped     proj_J 1.1 (relo)
    proj_reduce_one_over_z         proj_J 1.6e3 (ex_td_tr)
    prior_sign_flip_dropped        prior_r 1.0 (old_K11_n75/antipodal)
    prior_factor_2_dropped         prior_r 5.0e-1 (old_K4_ex_td/rot179)
    prior_sb_6_of_9                prior_r 5.5e-1 (old_K4_ex_td/dx0.3)"""


@pytest.fixture(scope="session")
def E64():
    return {k: v[0] for k, v in R.yardstick().items()}


def _held(err, E64, what, tag, suffix=''):
    print(f"factor_error {tag} {what}: " + "  ".join(f"{k + suffix} {v:.2e} = {v / E64[k]:.2f} x E64" for k, v in err.items()))
    for k, v in err.items():
        assert v <= M[k + suffix] * E64[k], f"{what} {k + suffix}: {v:.3e} > {M[k + suffix]} x {E64[k]:.3e}"
    return err


# ---- the device checks, one body for the emulator and the MI355X ------------------------------------------------------------------
def check_imu(h, E64, tag, mode):
    """every IMU case in one info mode; the absent factor between two cases of a window and the skipped one (sum_dt > 10) stay zero"""
    suffix = '_refinfo' if mode == ba.VG_IMU_INFO_REFERENCE else ''
    h.ba_set_imu_info_mode(mode)
    try:
        outs = [(h.ba_eval_factors(prob), pair) for prob, pair in R.imu_windows()]
    finally:
        h.ba_set_imu_info_mode(ba.VG_IMU_INFO_FACTOR)
    seen = 0
    for out, pair in outs:
        for slot, name in enumerate(pair):
            if name is None:
                continue
            got = dict(r=out['imu_r'][2 * slot], J=out['imu_J'][2 * slot])
            ref = R.imu_reference(name)
            err = R.imu_error(got, ref, R.imu_is_far(name))
            if ref is None:
                assert err == dict(imu_J=0.0, imu_r=0.0), f"{name}: a skipped factor's rows are not zero"
                print(f"factor_error {tag} {name}{suffix}: skipped, rows exactly zero")
            else:
                _held(err, E64, name, tag, suffix)
            seen += 1
        if pair[1] is not None:
            assert not out['imu_r'][1].any() and not out['imu_J'][1].any(), f"{pair}: the absent factor's rows are not zero"
    assert seen == len(R.imu_cases())


def check_proj(h, E64, tag):
    for wname, prob in R.proj_windows().items():
        out = h.ba_eval_factors(prob)
        refs, names = R.proj_reference(wname), R.proj_factor_names(wname)
        assert len(refs) == len(names) == out['proj_r'].shape[0]
        for f, k in enumerate(R.device_order(prob)):
            _held(R.proj_error(dict(r=out['proj_r'][f], J=out['proj_J'][f]), refs[k]), E64, names[k], tag)
        if not prob['estimate_td']:
            assert not out['proj_J'][:, :, 19].any()


def check_prior(h, E64, tag):
    for name, prob in R.prior_cases().items():
        out = h.ba_eval_factors(prob)
        _held(R.prior_error(out['prior_r'], R.prior_reference(name), R.prior_is_x0(name)), E64, name, tag)
        if name == 'dyadic/at_x0':
            assert np.array_equal(out['prior_r'], prob['prior']['r0']), f"{name}: prior_r is not r0 bit for bit"


# ---- the reference, the table and the bound themselves (no device) ----------------------------------------------------------------
def test_float64_restatement_is_the_oracle():
    """factor_ref in float64 repeats B.imu_factor / projection_factor / projection_td_factor / prior_factor bit for bit: the edits
    below are edits of the oracle."""
    for name, c in R.imu_cases().items():
        mine = R.imu_float64(name)
        r, Js = B.imu_factor(c['pre'], c['pose_i'], c['sb_i'], c['pose_j'], c['sb_j'], R.G_NORM)
        assert np.array_equal(mine['r'], r) and np.array_equal(mine['J'], np.hstack(Js)), name
    for wname, prob in R.proj_windows().items():
        st, K = B.state_of(prob), prob['pose'].shape[0]
        for mine, (l, fi, fj, oi, oj) in zip(R.proj_table(prob, np.float64), B.factor_list(prob)):
            pj = st['pose'][fj] if fj < K else st['relo_pose']
            if prob['estimate_td']:
                r, Js = B.projection_td_factor(st['pose'][fi], pj, st['ex'], st['inv_depth'][l], st['td'], oi, oj, prob['focal'], prob['tr'], prob['row'])
                assert np.array_equal(mine['J'][:, 19], Js[4][:, 0]), (wname, l, fj)
            else:
                r, Js = B.projection_factor(st['pose'][fi], pj, st['ex'], st['inv_depth'][l], np.array([oi[0], oi[1], 1.0]), np.array([oj[0], oj[1], 1.0]),
                                            prob['focal'])
                assert not mine['J'][:, 19].any()
            assert np.array_equal(mine['r'], r) and np.array_equal(mine['J'][:, :19], np.hstack(Js[:4])), (wname, l, fj)
    for name, prob in R.prior_cases().items():
        st = B.state_of(prob)
        r, _ = B.prior_factor(prob['prior'], [B.get_block(st, k, i) for (k, i) in prob['prior']['blocks']])
        assert np.array_equal(R.prior_table(prob, np.float64)['r'], r), name


def test_upper_factor_is_the_sqrt_info_of_the_reference():
    """U U^T = covariance and W = U^-1 upper triangular with W^T W covariance = I, in 80 bits, on the worst-conditioned record"""
    cov = np.asarray(R.imu_record('n99_dt0.1')['covariance'], np.float64).astype(R.LD).reshape(15, 15)
    U = R.upper_factor(cov)
    W = R.upper_inverse(U)
    assert np.array_equal(U, np.triu(U)) and np.array_equal(W, np.triu(W))
    scale = np.sqrt(np.outer(np.diag(cov), np.diag(cov)))
    assert float(np.triu(np.abs(U @ U.T - cov) / scale).max()) < 2.0 ** -58     # (the upper triangle is what is read, here and on the device)
    assert float(np.abs(W @ U - np.eye(15)).max()) < 2.0 ** -50 and np.linalg.cond(cov.astype(float)) > 1e8
    # the float64 route (inverse, then LLT) gives the same factor as far as float64 carries it
    W64 = B.imu_sqrt_info(cov.astype(np.float64))
    assert float(np.abs(U @ W64.astype(R.LD) - np.eye(15)).max()) < 1e-6


def test_case_table():
    """The table holds what the checks are for: every record x state of the IMU cases, every landmark x configuration, every prior x
    state (a case taken out fails here)."""
    imu = R.imu_cases()
    assert len(imu) == 6 * 12 + 1 and len(R.imu_windows()) == 37
    for rec in R.IMU_RECORDS[:-1]:
        for st in R.IMU_STATES:
            assert f"{rec}/{'/'.join(st)}" in imu
    assert len(R.IMU_STATES) == 12 and [n for n in imu if n.startswith(R.IMU_SKIPPED)] == ['n120_dt0.1/perturbed/bias1e-4/plain']
    assert set(R.proj_windows()) == {'plain', 'ex', 'td', 'ex_td_tr', 'relo'}
    assert set(R.PROJ_LANDMARKS) == {'lambda1e-4', 'lambda1e-3', 'lambda0.2', 'lambda20', 'image_edge', 'z_j0.1', 'td_plus_minus', 'td_minus_plus',
                                     'row_top', 'row_bottom', 'velocity0'}
    for w in R.PROJ_CONFIGS:
        assert len(R.proj_factor_names(w)) == 2 * len(R.PROJ_LANDMARKS) - 1
    assert set(R.priors()) == {'old_K4', 'old_K4_ex_td', 'second_new_K4', 'old_K11_n75', 'dyadic'}
    assert len(R.prior_cases()) == 5 * 5 and R.PRIOR_STATES == ('at_x0', 'dx1e-3', 'dx0.3', 'antipodal', 'rot179')


def test_case_properties():
    check_case_properties()


def check_case_properties():
    """each case reaches what it is there for, asserted from the reference (no device)"""
    imu = R.imu_cases()
    for name, c in imu.items():
        ref, (consistency, bias, special) = R.imu_reference(name), c['state']
        if c['record'] == R.IMU_SKIPPED:
            assert ref is None and c['pre']['sum_dt'] > 10.0
            continue
        assert c['pre']['sum_dt'] <= 10.0
        raw = np.abs(ref['r_raw'].astype(float))
        db = max(np.abs(c['sb_i'][3:6] - c['pre']['lin_ba']).max(), np.abs(c['sb_i'][6:9] - c['pre']['lin_bg']).max())
        assert {'bias0': db == 0.0, 'bias1e-4': 5e-5 < db < 1.1e-4, 'bias_far': 0.1 < db < 0.31}[bias], (name, db)
        if special in ('plain', 'antipodal', 'far_position'):
            if consistency == 'consistent':                         # rounding noise and the bias random walk, nothing else
                assert raw[0:3].max() < 1e-9 * max(1.0, ref['scale'][0]) and raw[3:6].max() < 1e-12 and raw[6:9].max() < 1e-10 * max(1.0, ref['scale'][2]), (name, raw)
            else:
                assert 0.2 < np.linalg.norm(raw[0:3]) < 0.8 and 0.15 < np.linalg.norm(raw[3:6]) < 0.25 and 0.5 < np.linalg.norm(raw[6:9]) < 1.5, (name, raw)
        if special == 'rot178':
            angle = 2 * np.degrees(np.arctan2(np.linalg.norm(raw[3:6]) / 2, abs(ref['qe_w'])))
            assert angle > (177.9 if consistency == 'consistent' else 160.0), (name, angle)   # a relative rotation near 180 degrees
        if special == 'far_position':
            assert np.abs(c['pose_i'][:3]).max() >= 9e4
    assert 9.8 < R.imu_record('n99_dt0.1')['sum_dt'] < 10.0
    c = R.IR.CASES['n1']                                          # why the one-sample record is not in the table: no weight exists
    assert np.linalg.matrix_rank(R.IR.oracle64(c['iv'], c['ba'], c['bg'], c['noise'])['covariance']) == 12
    # the antipodal Q_j: w < 0 in the residual's quaternion, and the residual is the NEGATED one (IMUFactor has no sign flip)
    for rec in R.IMU_RECORDS[:-1]:
        name = f"{rec}/perturbed/bias_far/antipodal"
        c, ref = imu[name], R.imu_reference(name)
        flipped = R.imu_factor(c['pre'], c['pose_i'], c['sb_i'], np.concatenate([c['pose_j'][:3], -c['pose_j'][3:]]), c['sb_j'])
        assert ref['qe_w'] < 0 < flipped['qe_w'] and np.array_equal(ref['r_raw'][3:6], -flipped['r_raw'][3:6]) and np.abs(ref['r_raw'][3:6]).max() > 0.05
    # projection: the depths, the edge, the zero baseline, the td / row terms
    for wname in R.PROJ_CONFIGS:
        prob, refs, names = R.proj_windows()[wname], R.proj_reference(wname), R.proj_factor_names(wname)
        assert prob['pose'].shape[0] == 3 and len(prob['inv_depth']) <= 16
        assert np.array_equal(prob['pose'][0][:3], prob['pose'][1][:3]) and not np.array_equal(prob['pose'][0][3:], prob['pose'][1][3:])
        lam = dict(zip(R.PROJ_LANDMARKS, prob['inv_depth']))
        assert [lam[k] for k in ('lambda1e-4', 'lambda1e-3', 'lambda0.2', 'lambda20')] == [1e-4, 1e-3, 0.2, 20.0]
        dep = {n: r['dep_j'] for n, r in zip(names, refs)}
        assert abs(dep[f'{wname}/z_j0.1/0-2'] - 0.1) < 1e-3 and all(d > 0.04 for d in dep.values()), dep
        o = prob['obs'][int(prob['obs_off'][list(R.PROJ_LANDMARKS).index('image_edge')])]
        assert abs(o[2] - 752) < 20 and abs(o[3] - 480) < 20       # the first observation lies in the image's corner
        for lm, v in (('row_top', 0.0), ('row_bottom', 479.0)):
            assert np.all(prob['obs'][int(prob['obs_off'][list(R.PROJ_LANDMARKS).index(lm)]):][:3, 3] == v)
        if prob['estimate_td']:
            oi = prob['obs'][int(prob['obs_off'][list(R.PROJ_LANDMARKS).index('td_plus_minus')])]
            oj = prob['obs'][int(prob['obs_off'][list(R.PROJ_LANDMARKS).index('td_plus_minus')]) + 1]
            assert np.isclose(prob['td'] - oi[6], 0.03) and np.isclose(prob['td'] - oj[6], -0.03)
            for n, r in zip(names, refs):
                assert bool(r['J'][:, 19].any()) == ('velocity0' not in n), n
    assert R.proj_windows()['ex_td_tr']['tr'] == 0.02 and R.proj_windows()['ex_td_tr']['row'] == 480.0 and R.proj_windows()['td']['tr'] == 0.0
    assert len(R.relo_window()['relo']['match']) == 8
    # prior: at x0 the reference's dx is exactly zero; dq.w < 0 in the antipodal case and only there (and past 180 degrees nowhere)
    for name, prob in R.prior_cases().items():
        ref, state = R.prior_reference(name), name.split('/')[1]
        assert len(ref['dq_w']) >= (1 if name.startswith('dyadic') else 2)
        if name == 'dyadic/at_x0':
            assert not ref['dx'].any() and np.array_equal(ref['r'].astype(float), prob['prior']['r0'])
            assert not R.prior_table(prob, np.float64)['dx'].any()
        elif state == 'at_x0':                                      # q0^-1 q0 leaves rounding residue in every number format
            assert 0 < np.abs(ref['dx'].astype(float)).max() < 1e-18 and 0 < np.abs(R.prior_table(prob, np.float64)['dx']).max() < 1e-15
        elif state == 'antipodal':
            assert all(w < -0.99 for w in ref['dq_w'])
        else:
            assert all(w > 0 for w in ref['dq_w'])
        if state == 'rot179':
            assert min(ref['dq_w']) < 0.01 and np.abs(ref['dx']).max() > 1.0
        if state in ('dx1e-3', 'dx0.3'):
            mag = float(state[2:])
            assert 0.2 * mag < np.abs(ref['dx'].astype(float)).max() < 5 * mag


def test_yardstick(E64):
    """E64 per kind is rounding noise of float64 times the kind's conditioning, nothing else (a reference or a metric gone wrong would
    show here).  Conditioning: the projection through a point 5 cm in front of a camera half a metre from the body origin amplifies
    by ~ |p| / z; the IMU kinds pass through U W64 - I of a covariance with cond 1e9, whose rows the metric holds against the raw
    blocks (measured: a few dozen roundings); the prior's sum is measured against the sum of its terms' magnitudes: n roundings."""
    for k, (v, name) in R.yardstick().items():
        print(f"E64 {k}: {v:.3e} ({name})")
    for name in R.case_names():
        print(f"e64 {name}: ", {k: f"{v:.2e}" for k, v in R.e64(name).items()})
    cond = R.conditioning()
    print("conditioning:", {k: f"{v:.3g}" for k, v in cond.items()})
    for k in R.KINDS:
        assert 2.0 ** -53 < E64[k] < 4 * cond[k] * 2.0 ** -52, (k, E64[k], cond[k])
    assert all(m in (1, 2, 4, 8, 16, 32, 64) for m in M.values())


def test_metric_sees_what_the_old_one_did_not():
    """the raw dp/dba_i block of the reference times 1.001, re-weighted: test_factor_parity's atol = 1e-6 of the row weight passes
    it, the block's own scale shows 1e-3"""
    name = 'n2/perturbed/bias1e-4/plain'
    ref = R.imu_reference(name)
    Jraw = ref['J_raw'].copy()
    Jraw[0:3, 9:12] = Jraw[0:3, 9:12] * R.LD(1.001)
    got = dict(r=ref['r'].astype(np.float64), J=(ref['W'] @ Jraw).astype(np.float64))
    W = B.imu_sqrt_info(np.asarray(R.imu_cases()[name]['pre']['covariance']).reshape(15, 15))
    scale = np.abs(W).sum(axis=1)
    assert np.allclose(got['J'] / scale[:, None], ref['J'].astype(np.float64) / scale[:, None], atol=1e-6)
    assert np.allclose(got['J'] / scale[:, None], R.imu_float64(name)['J'] / scale[:, None], atol=1e-6)
    err = R.imu_error(got, ref)
    assert err['imu_J'] > 1e-4 and err['imu_r'] < 1e-15, err


@pytest.mark.parametrize("edit", R.EDITS)
def test_each_edit_exceeds_twice_the_bound(E64, edit):
    names = list(R.imu_cases()) if edit in R.IMU_EDITS else list(R.proj_windows()) if edit in R.PROJ_EDITS else list(R.prior_cases())
    worst = {}
    for name in names:
        for k, v in R.e64(name, edit).items():
            if v > worst.get(k, (0.0, None))[0]:
                worst[k] = (v, name)
    print(f"edit {edit}: " + "  ".join(f"{k} {v[0]:.2e} ({v[1]})" for k, v in worst.items()))
    assert any(v[0] > 2 * max(M[k], M.get(k + '_refinfo', 0)) * E64[k] for k, v in worst.items()), worst


# ---- emulated kernels (CPU fiber emulator) ----------------------------------------------------------------------------------------
def test_emulated_imu(simt_handle, E64):
    check_imu(simt_handle, E64, 'emulated', ba.VG_IMU_INFO_FACTOR)


def test_emulated_imu_reference_info(simt_handle, E64):
    check_imu(simt_handle, E64, 'emulated', ba.VG_IMU_INFO_REFERENCE)


def test_emulated_projection(simt_handle, E64):
    check_proj(simt_handle, E64, 'emulated')


def test_emulated_prior(simt_handle, E64):
    check_prior(simt_handle, E64, 'emulated')


# ---- MI355X -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_imu(handle, E64):
    check_imu(handle, E64, 'gpu', ba.VG_IMU_INFO_FACTOR)


@pytest.mark.gpu
def test_imu_reference_info(handle, E64):
    check_imu(handle, E64, 'gpu', ba.VG_IMU_INFO_REFERENCE)


@pytest.mark.gpu
def test_projection(handle, E64):
    check_proj(handle, E64, 'gpu')


@pytest.mark.gpu
def test_prior(handle, E64):
    check_prior(handle, E64, 'gpu')
