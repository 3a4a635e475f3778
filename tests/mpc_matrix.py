"""The compiled instances of the MPC search kernel (csrc/abr_env.hip: mpc_select_kernel<H, BC, WVM>) and one table of
cases that reaches every one of them.  Shared by the ISA coverage check (test_rules_cpu.py) and the GPU parity tests
(test_mpc_instances_gpu.py), so an instance added to or removed from launch_mpc fails on the CPU until the table
covers it."""
import re


def mpc_instance(B, H, wv):
    """launch_mpc's dispatch as data: (n_rates, horizon, variance_weight) -> (H, BC, WVM) of the instance it launches.
    BC = 0 is the generic rate count; WVM 1 drops the multiplication by a weight of exactly 1.0, WVM 2 the whole
    variance term for a weight of exactly 0.0 (-0.0 included: it compares equal)."""
    if H <= 6:
        if B == 6 and wv == 1.0:
            return (H, 6, 1)
        if B == 6 and wv == 0.0:
            return (H, 6, 2)
        if B == 6:
            return (H, 6, 0)
        if B == 4 and wv == 0.0:
            return (H, 4, 2)
        if B == 4:
            return (H, 4, 0)
        if B in (5, 3, 8, 7):
            return (H, B, 0)
    return (H, 0, 0)


def lanes_per_block(B, H):
    """launch_mpc_b: lanes per workgroup for T = B^D threads per lane (D = 2 from horizon 3 on)."""
    T = B * B if H >= 3 else B
    return max(1, min(16, 256 // T))


# (B, H, wv): at least one case per instance.  The generic instance of each horizon is reached by a rate count that
# has no specialisation (2, or 9 and above); horizons 7 and 8 have only the generic one.
_GENERIC_B = {2: 16, 3: 10, 4: 9, 5: 2, 6: 2, 7: 3, 8: 2}
MPC_CASES = []
for _H in range(2, 7):
    MPC_CASES += [(6, _H, 1.0), (6, _H, 0.0), (6, _H, 0.5), (4, _H, -0.0), (4, _H, 1.0), (5, _H, 1.0),
                  (3, _H, 0.5), (8, _H, 1.0), (7, _H, 2.0), (_GENERIC_B[_H], _H, 1.0)]
MPC_CASES += [(_GENERIC_B[7], 7, 1.0), (_GENERIC_B[8], 8, 0.5)]


def case_id(case):
    B, H, wv = case
    return "B%d-H%d-wv%s" % (B, H, repr(wv))


def instance_name(inst):
    return "<%d,%d,%d>" % inst


def isa_instances(asm_text):
    """The (H, BC, WVM) of every mpc_select_kernel symbol defined in `make asm`'s output."""
    return {tuple(int(x) for x in m) for m in
            re.findall(r"^\s*\.amdhsa_kernel\s+_Z17mpc_select_kernelILi(\d+)ELi(\d+)ELi(\d+)E", asm_text, re.M)}
