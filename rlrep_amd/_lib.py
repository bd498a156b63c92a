"""ctypes binding of librlrep_hip.so (the C ABI declared in include/rlrep.h).

There is NO fallback: if the HIP library is missing or fails to load, importing this module raises.
`import torch` must happen first so that the library resolves libamdhip64.so.7 to the HIP runtime
torch already loaded (device pointers and streams are shared with torch).
"""
import ctypes as C
import os
import re

import torch  # noqa: F401  (must precede the CDLL load, see docstring)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('RLREP_LIB') or os.path.join(_HERE, 'lib', 'librlrep_hip.so')     # RLREP_LIB: A/B builds of the same ABI
HEADER_PATH = os.path.join(os.path.dirname(_HERE), 'include', 'rlrep.h')

ALG = {'sac': 0, 'vlsac': 1, 'ctrlsac': 2, 'spedersac': 3, 'diffsrsac': 4}
ARENA_PARAM, ARENA_TARGET = 0, 1
GRAD_TAIL = 256
FLAG_NO_FEATURE_TARGET = 1


class Dims(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        'alg', 'state_dim', 'action_dim', 'hidden_dim', 'actor_hidden_dim', 'feature_dim', 'vae_hidden_dim',
        'phi_hidden_dim', 'phi_hidden_depth', 'mu_hidden_dim', 'mu_hidden_depth', 'num_noise', 'max_batch', 'rank', 'flags', 'world_size')]


class Hyper(C.Structure):
    _fields_ = [('lr_feature', C.c_float), ('lr_critic', C.c_float), ('lr_actor', C.c_float),
                ('discount', C.c_float), ('tau', C.c_float), ('feature_tau', C.c_float),
                ('target_entropy', C.c_float), ('sigma_scale', C.c_float),
                ('target_update_period', C.c_int32), ('extra_feature_steps', C.c_int32),
                ('learn_alpha', C.c_int32), ('world_size', C.c_int32),
                ('beta1', C.c_float), ('beta2', C.c_float), ('adam_eps', C.c_float), ('critic_reg_lambda', C.c_float)]


class TensorDesc(C.Structure):
    _fields_ = [('name', C.c_char * 72), ('arena', C.c_int32), ('group', C.c_int32), ('offset', C.c_int64),
                ('rows', C.c_int32), ('cols', C.c_int32)]


class LayoutInfo(C.Structure):
    _fields_ = [('param_floats', C.c_int64), ('target_floats', C.c_int64), ('grad_floats', C.c_int64),
                ('workspace_bytes', C.c_int64), ('group_offset', C.c_int64 * 4), ('group_floats', C.c_int64 * 4),
                ('n_tensors', C.c_int32), ('n_metrics', C.c_int32), ('exchange_floats', C.c_int64)]


class Arenas(C.Structure):
    _fields_ = [('param_dev', C.c_void_p), ('target_dev', C.c_void_p), ('grad_dev', C.c_void_p),
                ('exp_avg_dev', C.c_void_p), ('exp_avg_sq_dev', C.c_void_p), ('workspace_dev', C.c_void_p),
                ('alpha_state_dev', C.c_void_p)]


class Batch(C.Structure):
    _fields_ = [('state_dev', C.c_void_p), ('action_dev', C.c_void_p), ('reward_dev', C.c_void_p),
                ('next_state_dev', C.c_void_p), ('done_dev', C.c_void_p), ('batch', C.c_int32)]


class Gemm16Task(C.Structure):
    """rlrep_gemm16_task (include/rlrep.h): one product of a rlrep_gemm16_table launch."""
    _fields_ = [('a', C.c_void_p), ('b', C.c_void_p), ('c', C.c_void_p),
                ('lda', C.c_int32), ('ldb', C.c_int32), ('ldc', C.c_int32), ('rows', C.c_int32), ('cols', C.c_int32), ('inner', C.c_int32),
                ('epi', C.c_int32), ('act', C.c_int32), ('flags', C.c_int32),
                ('bias', C.c_void_p), ('aux', C.c_void_p), ('ldaux', C.c_int32), ('out2', C.c_void_p),
                ('r1u', C.c_void_p), ('r1v', C.c_void_p), ('scale', C.c_float)]


class SimState(C.Structure):
    """rlrep_sim_state (include/rlrep.h): the arrays of a fused simulator (envs/fused_sim.py); rlrep_sim_state_bytes() is its size."""
    _fields_ = [(n, C.c_void_p) for n in ('x0', 'x1', 'ep_return', 'last_return', 't', 'episodes', 'starts', 'obs')] + [
        ('kind', C.c_int32), ('n', C.c_int32), ('seed', C.c_uint64), ('auto_restart', C.c_int32), ('reserved', C.c_int32)]


class SimKindDesc(C.Structure):
    """rlrep_sim_kind_desc (include/rlrep.h): a simulator kind given as text (envs/fused_sim.py SimKind)."""
    _fields_ = [('name', C.c_char_p), ('source', C.c_char_p), ('S', C.c_int32), ('A', C.c_int32), ('NX', C.c_int32), ('limit', C.c_int32),
                ('terminates', C.c_int32), ('reserved', C.c_int32)]


class SimKindInfo(C.Structure):
    """rlrep_sim_kind_info_t (include/rlrep.h): a compiled kind's constants and, per kernel, registers / scratch bytes / static LDS bytes."""
    _fields_ = [('S', C.c_int32), ('A', C.c_int32), ('NX', C.c_int32), ('limit', C.c_int32), ('terminates', C.c_int32), ('reserved', C.c_int32),
                ('regs', C.c_int32 * 3), ('scratch_bytes', C.c_int32 * 3), ('lds_bytes', C.c_int32 * 3)]


class SimxState(C.Structure):
    """rlrep_simx_state (include/rlrep.h): the arrays of a fused simulator of a compiled kind; rlrep_simx_state_bytes() is its size."""
    _fields_ = [(n, C.c_void_p) for n in ('x', 'ep_return', 'last_return', 't', 'episodes', 'starts', 'obs')] + [
        ('n', C.c_int32), ('auto_restart', C.c_int32), ('seed', C.c_uint64)]


RL_KERNEL = {'infonce': 0, 'score_infonce': 1, 'colsum': 2, 'speder_rows': 3, 'speder_grads': 4, 'perturb': 5, 'score': 6, 'reg_stats': 7, 'copy2': 8}
SCORE_FORM = ('LDS32', 'LDS64', 'LDS128', 'SMALL1', 'SMALL2', 'SMALL4', 'VEC', 'ROWS')          # RLREP_SCORE_* of include/rlrep.h, by value


def _rec(spec):
    """ctypes fields from 'p:a,b i:c f:d' (p pointer, i int32, f float, l int64), in declaration order"""
    kinds = {'p': C.c_void_p, 'i': C.c_int32, 'f': C.c_float, 'l': C.c_int64}
    return [(n, kinds[part[0]]) for part in spec.split() for n in part[2:].split(',')]


class _RlInfoNce(C.Structure):
    _fields_ = _rec('p:S i:ldS,ncols,diag_off p:rhat,r,drhat,partial i:B f:inv_batch p:Z i:ldZ,F p:theta_w,theta_b,ZM i:ldZM')


class _RlColSum(C.Structure):
    _fields_ = _rec('p:X i:ldX p:w,out i:rows,F p:X2 i:ldX2 p:w2,out2,outb2 i:rows2')


class _RlSpederRows(C.Structure):
    _fields_ = _rec('p:phi,mu,mu_r,phibar,theta_w,theta_b,r,c,drhat,partial i:B,F f:inv_batch')


class _RlSpederGrads(C.Structure):
    _fields_ = _rec('p:phi,mu,c,drhat,phibar,v,theta_w,Gphi,Gmu i:B,F f:inv_batch')


class _RlPerturb(C.Structure):
    _fields_ = _rec('p:alphabars,idx,s2 i:ld_s2 p:eps,XN,TGT i:B,S')


class _RlScore(C.Structure):
    _fields_ = _rec('p:U,PHI,TGT,alphabars,idx,GPHI,partial i:B,F,S f:sigma,inv_batch')


class _RlRegStats(C.Structure):
    _fields_ = [('X', C.c_void_p * 4), ('C', C.c_void_p * 4)] + _rec('i:B,H f:lam p:partial')


class _RlCopy2(C.Structure):
    _fields_ = _rec('p:src,d1,d2 l:n')


class ReplearnArgs(C.Union):
    """rlrep_replearn_args (include/rlrep.h): the record of one rlrep_replearn launch (reg_stats.lam is the header's `lambda`)."""
    _fields_ = [('infonce', _RlInfoNce), ('colsum', _RlColSum), ('speder_rows', _RlSpederRows), ('speder_grads', _RlSpederGrads),
                ('perturb', _RlPerturb), ('score', _RlScore), ('reg_stats', _RlRegStats), ('copy2', _RlCopy2)]


NC_KERNEL = {'fwd': 0, 'dx': 1, 'dw': 2}                                          # RLREP_NC_* of include/rlrep.h


class NcFwdTask(C.Structure):
    """rlrep_nc_fwd_task (include/rlrep.h)"""
    _fields_ = _rec('p:mean,lstd i:ld_ml p:noise,W,bias,w3,Hm,U,sigma_out i:B,F,H')


class NcDwTask(C.Structure):
    """rlrep_nc_dw_task (include/rlrep.h)"""
    _fields_ = _rec('p:U,GH i:ldgh p:mean,sigma i:ld_ml p:noise,gW,gb i:B,F,H')


class _NcFwd(C.Structure):
    _fields_ = _rec('i:ntasks,g2,cols') + [('form', C.POINTER(C.c_int32)), ('t', NcFwdTask * 4)]


class _NcDx(C.Structure):
    _fields_ = ([('GH', C.c_void_p * 2)] + _rec('i:ldgh') + [('U', C.c_void_p * 2), ('W', C.c_void_p * 2)] + _rec('p:noise,lstd i:ld_l p:G i:ldg,B,F,H,nheads')
                + [('form', C.POINTER(C.c_int32))])


class _NcDw(C.Structure):
    _fields_ = _rec('i:ntasks,lean,splits p:slab l:slab_floats p:bslab l:bslab_floats') + [('form', C.POINTER(C.c_int32)), ('t', NcDwTask * 2)]


class NoisecriticArgs(C.Union):
    """rlrep_noisecritic_args (include/rlrep.h): the record of one rlrep_noisecritic launch"""
    _fields_ = [('fwd', _NcFwd), ('dx', _NcDx), ('dw', _NcDw)]


HD_KIND = {'policy_fwd': 0, 'policy_bwd': 1, 'vae_mid': 2, 'heads_vae': 3, 'vae_mse': 4, 'reparam_dx': 5, 'qhead_critic': 6, 'qhead_actor': 7}   # RLREP_HD_* of include/rlrep.h
_FORM = [('form', C.POINTER(C.c_int32))]


class HdLayer(C.Structure):
    """rlrep_hd_layer (include/rlrep.h): the layer whose epilogue a fused head is"""
    _fields_ = _rec('p:X i:ldx p:W i:ldw p:bias i:K')


class HdPolicyTask(C.Structure):
    """rlrep_hd_policy_task (include/rlrep.h)"""
    _fields_ = _rec('p:O,eps,act i:ld_act p:logp') + [('l', HdLayer)]


class _HdExtra(C.Structure):
    _fields_ = [('l', HdLayer)] + _rec('p:Y i:ldy,rows,N,act')


class _HdPolicyFwd(C.Structure):
    _fields_ = _rec('i:fused,ntasks,B,A,clamp f:lo,hi') + _FORM + [('t', HdPolicyTask * 2), ('extra', _HdExtra)]


class _HdPolicyBwd(C.Structure):
    _fields_ = _rec('i:fused p:O,eps,act i:ld_act p:dA i:ld_dA p:alpha_state f:inv_batch p:G i:B,A') + _FORM + [('l', HdLayer)]


class _HdVaeMid(C.Structure):
    _fields_ = _rec('p:EH,FH,eps,Z,EZ,GEH,GFH,partial i:B,F f:scale') + _FORM


class _HdHeadsVae(C.Structure):
    _fields_ = _rec('p:Ae,Af i:lda p:We,be,Wf,bf,eps,Z,EZ,GEH,GFH,partial,EH,FH i:B,F,K f:scale') + _FORM


class _HdVaeMse(C.Structure):
    _fields_ = _rec('i:fused p:DH,s2 i:ld_s2 p:r,GDH,partial i:B,S f:scale_s,scale_r') + _FORM + [('l', HdLayer)]


class _HdReparamDx(C.Structure):
    _fields_ = _rec('i:pre p:A i:lda p:W i:ldw p:G i:ldg p:EZ i:ldez,B,F,K p:X i:ldx p:Wh i:ldwh,K1 p:M i:ldm p:bh,s2 i:ld_s2 p:r f:scale_s,scale_r p:partial') + _FORM


class _HdQheadCritic(C.Structure):
    _fields_ = ([(n, C.c_void_p * 2) for n in ('Et', 'Ec', 'wt', 'bt', 'wc', 'bc')] + _rec('p:logp,R,D,alpha_state f:gamma,inv_batch p:dq')
                + [('GE', C.c_void_p * 2)] + _rec('p:partial i:B,H,train,ldE,weighted p:w,td') + _FORM)


class _HdQheadActor(C.Structure):
    _fields_ = ([(n, C.c_void_p * 2) for n in ('Ec', 'wc', 'bc')] + _rec('p:logp,alpha_state f:inv_batch,target_entropy')
                + [('GE', C.c_void_p * 2)] + _rec('p:partial_loss,partial_c i:B,H,ldE') + _FORM)


class HeadsArgs(C.Union):
    """rlrep_heads_args (include/rlrep.h): the record of one rlrep_heads launch"""
    _fields_ = [('policy_fwd', _HdPolicyFwd), ('policy_bwd', _HdPolicyBwd), ('vae_mid', _HdVaeMid), ('heads_vae', _HdHeadsVae), ('vae_mse', _HdVaeMse),
                ('reparam_dx', _HdReparamDx), ('qhead_critic', _HdQheadCritic), ('qhead_actor', _HdQheadActor)]


def declared_symbols():
    """Every function name include/rlrep.h declares (used by the CPU test that checks the exports)."""
    src = open(HEADER_PATH).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(rlrep_[a-z_0-9]+)\s*\(', src)))


def _load():
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f'{LIB_PATH} is missing: build it with `python -c "import __graft_entry__ as g; g.build()"` '
            f'(hipcc --offload-arch=gfx950).  rlrep_amd has no CPU fallback.')
    lib = C.CDLL(LIB_PATH)
    vp, i32, i64, u64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_float
    P = C.POINTER
    sig = {
        'rlrep_abi_version': (i32, []),
        'rlrep_last_error': (C.c_char_p, []),
        'rlrep_layout': (i32, [P(Dims), P(LayoutInfo), P(TensorDesc), i32]),
        'rlrep_metric_names': (i32, [i32, vp, i32]),
        'rlrep_agent_create': (i32, [P(Dims), P(Hyper), P(Arenas), vp, P(vp)]),
        'rlrep_agent_destroy': (None, [vp]),
        'rlrep_group_create': (i32, [P(Dims), P(Hyper), P(Arenas), i32, i64, vp, P(vp)]),
        'rlrep_group_max_members': (i32, []),
        'rlrep_group_members': (i32, [vp]),
        'rlrep_group_set_seeds': (i32, [vp, vp, i32, vp]),
        'rlrep_group_set_member_hyper': (i32, [vp, i32, P(Hyper), vp]),
        'rlrep_group_get_member_hyper': (i32, [vp, i32, P(Hyper)]),
        'rlrep_group_clone_members': (i32, [vp, P(i32), P(i32), i32, vp]),
        'rlrep_group_set_live': (i32, [vp, P(i32), vp]),
        'rlrep_group_get_live': (i32, [vp, P(i32)]),
        'rlrep_group_train_prologue': (i32, [vp, vp, i64, vp, vp, i64, vp, i64, u64, u64, i32, vp]),
        'rlrep_group_prepare': (i32, [vp, i32]),
        'rlrep_group_select_action': (i32, [vp, vp, i32, u64, f32, f32, vp, vp]),
        'rlrep_group_replay_add_sized': (i32, [vp, i64, i32, i64, i32, i64, vp, i64, i64, vp, i32, vp]),
        'rlrep_group_env_create': (i32, [vp, i32, P(vp)]),
        'rlrep_group_env_destroy': (None, [vp]),
        'rlrep_group_env_reset': (i32, [vp, vp]),
        'rlrep_group_env_step': (i32, [vp, vp, vp, i64, i64, vp, f32, f32, f32, i64, vp]),
        'rlrep_group_env_evaluate': (i32, [vp, vp, i32, u64, vp, vp]),
        'rlrep_group_env_state': (i32, [vp, i32, vp, i64, i32, vp]),
        'rlrep_env_create': (i32, [vp, i32, u64, P(vp)]),
        'rlrep_env_destroy': (None, [vp]),
        'rlrep_env_reset': (i32, [vp, vp]),
        'rlrep_env_step': (i32, [vp, vp, vp, i64, vp, f32, f32, f32, i64, vp]),
        'rlrep_env_evaluate': (i32, [vp, vp, i32, u64, vp, vp]),
        'rlrep_env_state': (i32, [vp, i32, vp, i64, i32, vp]),
        'rlrep_prepare': (i32, [vp, i32]),
        'rlrep_group_env_create_n': (i32, [vp, i32, i32, P(vp)]),
        'rlrep_group_env_num_envs': (i32, [vp]),
        'rlrep_env_create_n': (i32, [vp, i32, u64, i32, P(vp)]),
        'rlrep_env_num_envs': (i32, [vp]),
        'rlrep_set_batch': (i32, [vp, i32, P(Batch), vp]),
        'rlrep_replay_row_floats': (i32, [P(Dims)]),
        'rlrep_replay_add': (i32, [vp, i64, i32, i64, vp, i64, vp]),
        'rlrep_replay_add_sized': (i32, [vp, i64, i32, i64, vp, i64, vp, i32, vp]),
        'rlrep_replay_sample': (i32, [vp, i32, vp, vp, i32, vp]),
        'rlrep_fill_indices': (i32, [vp, i64, i32, u64, u64, vp]),
        'rlrep_fill_normal': (i32, [vp, i64, f32, u64, u64, vp]),
        'rlrep_philox_raw': (i32, [vp, vp, i64, vp]),
        'rlrep_fill_indices_dev': (i32, [vp, i64, vp, u64, u64, vp, vp]),
        'rlrep_fill_normal_dev': (i32, [vp, i64, f32, u64, u64, vp, vp]),
        'rlrep_steps_dev': (vp, [vp]),
        'rlrep_group_cfg_dev': (vp, [vp]),
        'rlrep_feature_step': (i32, [vp, vp, vp, vp]),
        'rlrep_prefetch_policy': (i32, [vp, vp]),
        'rlrep_prefetch_policy_early': (i32, [vp, vp, vp]),
        'rlrep_prefetch_batch': (i32, [vp, vp, vp, i32]),
        'rlrep_prefetch_batch_slot': (i32, [vp, i32, vp, vp, i32]),
        'rlrep_train_prologue': (i32, [vp, vp, vp, vp, i64, vp, i64, u64, u64, u64, i32, vp]),
        'rlrep_critic_step': (i32, [vp, vp, vp]),
        'rlrep_actor_alpha_step': (i32, [vp, vp, vp]),
        'rlrep_update_target': (i32, [vp, vp]),
        'rlrep_begin_train': (i32, [vp, vp]),
        'rlrep_feature_backward': (i32, [vp, vp, vp, vp]),
        'rlrep_feature_apply': (i32, [vp, vp]),
        'rlrep_critic_backward': (i32, [vp, vp, vp]),
        'rlrep_critic_apply': (i32, [vp, vp]),
        'rlrep_actor_backward': (i32, [vp, vp, vp]),
        'rlrep_actor_apply': (i32, [vp, vp]),
        'rlrep_feature_exchange_count': (i32, [vp]),
        'rlrep_feature_exchange': (i32, [vp, i32, P(i32), P(vp), P(i64), P(i64)]),
        'rlrep_feature_backward_part': (i32, [vp, i32, vp, vp, vp]),
        'rlrep_defer_supported': (i32, [vp]),
        'rlrep_defer_snapshot': (i32, [vp, i32, vp, vp, vp]),
        'rlrep_defer_arm': (i32, [vp, i32, vp, vp]),
        'rlrep_deferred_critic_actor': (i32, [vp, i32, vp]),
        'rlrep_deferred_part': (i32, [vp, i32, i32, vp]),
        'rlrep_end_train': (i32, [vp]),
        'rlrep_sync_frozen': (i32, [vp, vp]),
        'rlrep_actor_forward': (i32, [vp, vp, i32, vp, f32, f32, vp, vp]),
        'rlrep_select_action': (i32, [vp, vp, i32, i32, u64, u64, f32, f32, vp, i32, vp]),
        'rlrep_select_action_n': (i32, [vp, vp, i32, i32, i32, u64, u64, f32, f32, vp, i32, vp]),
        'rlrep_group_select_action_n': (i32, [vp, vp, i32, i32, u64, f32, f32, vp, vp]),
        'rlrep_act_device': (i32, [vp, vp, i64, i32, i32, u64, u64, f32, f32, vp, i64, vp]),
        'rlrep_group_act_device': (i32, [vp, vp, i32, i32, u64, f32, f32, vp, vp]),
        'rlrep_replay_add_cols': (i32, [vp, i64, i32, i64, i32, i32, vp, i64, vp, i64, vp, i64, vp, vp, i64, vp, i32, vp]),
        'rlrep_group_replay_add_cols': (i32, [vp, i64, i32, i64, i32, i32, vp, i64, vp, i64, vp, i64, vp, vp, i64, i32, i64, vp, i32, vp]),
        'rlrep_act_device_ctl': (i32, [vp, vp, i64, i32, u64, f32, f32, vp, i64, vp, i64, f32, i64, vp]),
        'rlrep_replay_add_cols_ctl': (i32, [vp, i64, i32, i32, i32, vp, i64, vp, i64, vp, i64, vp, vp, i64, vp, vp, vp]),
        'rlrep_sim_state_bytes': (i32, []),
        'rlrep_sim_start': (i32, [P(SimState), vp]),
        'rlrep_sim_step': (i32, [P(SimState), vp, i64, vp, vp, vp, vp]),
        'rlrep_sim_step_append_ctl': (i32, [P(SimState), vp, i64, vp, i64, i32, vp, vp, vp]),
        'rlrep_group_act_device_ctl': (i32, [vp, vp, i32, f32, f32, vp, vp, i64, f32, i64, vp]),
        'rlrep_group_replay_add_cols_ctl': (i32, [vp, vp, i64, i32, i32, i32, vp, i64, vp, i64, vp, i64, vp, vp, i64, i64, vp, vp, vp]),
        'rlrep_group_sim_start': (i32, [vp, P(SimState), vp, vp]),
        'rlrep_group_sim_step': (i32, [vp, P(SimState), vp, vp, i64, vp, vp, vp, vp]),
        'rlrep_group_sim_step_append_ctl': (i32, [vp, P(SimState), vp, vp, i64, vp, i64, i32, i64, vp, vp, vp]),
        'rlrep_simx_state_bytes': (i32, []),
        'rlrep_sim_kind_compile': (i32, [P(SimKindDesc), P(vp)]),
        'rlrep_sim_kind_destroy': (None, [vp]),
        'rlrep_sim_kind_info': (i32, [vp, P(SimKindInfo)]),
        'rlrep_sim_kind_source': (i64, [P(SimKindDesc), vp, i64]),
        'rlrep_sim_kind_code': (i32, [P(SimKindDesc), C.c_char_p, vp, i64, P(i64)]),
        'rlrep_simx_start': (i32, [vp, P(SimxState), vp]),
        'rlrep_simx_step': (i32, [vp, P(SimxState), vp, i64, vp, vp, vp, vp]),
        'rlrep_simx_step_append_ctl': (i32, [vp, P(SimxState), vp, i64, vp, i64, i32, vp, vp, vp]),
        'rlrep_per_add': (i32, [vp, i64, vp, i64, i64, i64, vp]),
        'rlrep_per_rebuild': (i32, [vp, i64, vp]),
        'rlrep_per_sample': (i32, [vp, vp, i64, vp, vp, vp, i32, i32, u64, u64, vp, vp]),
        'rlrep_per_update': (i32, [vp, vp, i64, vp, vp, vp, i32, vp]),
        'rlrep_critic_step_weighted': (i32, [vp, vp, vp, vp]),
        'rlrep_per_td_dev': (vp, [vp]),
        'rlrep_per_sample_fill': (i32, [vp, vp, i64, vp, i64, vp, vp, vp, i32, i32, u64, u64, vp, vp]),
        'rlrep_critic_weights_arm': (i32, [vp, vp, vp]),
        'rlrep_per_update_td': (i32, [vp, i64, vp, vp, vp, i32, vp]),
        'rlrep_group_per_add': (i32, [vp, i64, vp, i32, i64, i64, i64, vp]),
        'rlrep_group_per_sample': (i32, [vp, vp, i64, vp, vp, vp, i32, i32, u64, i32, vp, i64, i64, vp]),
        'rlrep_group_per_update': (i32, [vp, vp, i64, vp, vp, vp, i32, vp]),
        'rlrep_group_critic_step_weighted': (i32, [vp, vp, vp, vp]),
        'rlrep_group_per_td_dev': (vp, [vp]),
        'rlrep_group_per_sample_fill': (i32, [vp, vp, i64, i64, vp, i64, vp, vp, vp, i32, i32, u64, i32, vp]),
        'rlrep_group_critic_weights_arm': (i32, [vp, vp, vp]),
        'rlrep_group_per_update_td': (i32, [vp, vp, i64, vp, vp, vp, i32, vp]),
        'rlrep_replay_sample_nstep': (i32, [vp, i32, vp, vp, i32, i64, vp, i32, i32, vp]),
        'rlrep_replay_gather_nstep': (i32, [vp, vp, i32, i32, i32, i64, vp, i32, i32, f32, vp, vp, vp, vp, vp, vp, vp]),
        'rlrep_group_replay_gather_nstep': (i32, [vp, vp, i64, vp, i32, i32, i64, vp, i32, i32, vp]),
        'rlrep_slot_dev': (vp, [vp, i32, i32]),
        'rlrep_set_critic_nstep': (i32, [vp, i32]),
        'rlrep_replay_sample_nstep_targets': (i32, [vp, i32, vp, vp, i32, i64, vp, i32, i32, vp]),
        'rlrep_replay_gather_nstep_targets': (i32, [vp, vp, i32, i32, i32, i64, vp, i32, i32, f32, vp, vp, vp, vp]),
        'rlrep_images_managed': (i32, [vp, i32]),
        'rlrep_refresh_images': (i32, [vp, vp]),
        'rlrep_feature_chain_next': (i32, [vp]),
        'rlrep_comm_create': (i32, [i32, i32, i64, i64, P(vp)]),
        'rlrep_comm_handle_bytes': (i32, []),
        'rlrep_comm_handle': (i32, [vp, vp, i32]),
        'rlrep_comm_connect': (i32, [vp, vp]),
        'rlrep_comm_connect_local': (i32, [vp, P(vp)]),
        'rlrep_comm_set_timeout': (i32, [vp, i64]),
        'rlrep_comm_arena': (vp, [vp]),
        'rlrep_comm_scratch': (vp, [vp]),
        'rlrep_comm_attach': (i32, [vp, vp, i64, i64, P(i32)]),
        'rlrep_comm_allreduce': (i32, [vp, i64, i64, vp, i32, i64, vp]),
        'rlrep_comm_allgather': (i32, [vp, i64, i64, vp]),
        'rlrep_comm_probe_fill': (i32, [vp, i64, i64, i32, vp]),
        'rlrep_comm_probe_value': (f32, [i32, i32, i64]),
        'rlrep_comm_probe_slots': (i32, [vp, i64, i32, vp, i64, vp]),
        'rlrep_comm_status': (i32, [vp, P(C.c_uint32), i32]),
        'rlrep_comm_fine_grained': (i32, [vp]),
        'rlrep_comm_debug_preset': (i32, [vp, i32, i32]),
        'rlrep_comm_destroy': (None, [vp]),
        'rlrep_stage_count': (i32, [vp, i32]),
        'rlrep_stage_name': (C.c_char_p, [vp, i32, i32]),
        'rlrep_run_stage': (i32, [vp, i32, i32, vp]),
        'rlrep_stage_info': (i32, [vp, i32, i32, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        'rlrep_gemm': (i32, [i32, i32, i32, vp, i32, vp, i32, vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, i32, vp, i32, i32, vp, i64, vp]),
        'rlrep_gemm16_table': (i32, [i32, i32, i32, P(Gemm16Task), i32, i32, i32, i32, vp]),
        'rlrep_gemm_plan': (i32, [i32] * 8 + [P(i32)] * 5),
        'rlrep_replearn': (i32, [i32, P(ReplearnArgs), vp]),
        'rlrep_diffsr_score_plan': (i32, [i32, i32, i32, P(i32)]),
        'rlrep_nc_fwd_plan': (i32, [i32] * 4 + [P(i32)] * 3),
        'rlrep_noisecritic': (i32, [i32, P(NoisecriticArgs), vp]),
        'rlrep_nc_w3_bytes': (i64, [i32, i32]),
        'rlrep_nc_forms': (i32, [i32] * 5 + [P(i32)] * 2),
        'rlrep_heads': (i32, [i32, P(HeadsArgs), vp]),
        'rlrep_heads_partials': (i32, [i32] * 4),
        'rlrep_heads_plan': (i32, [i32, P(HeadsArgs)]),
        'rlrep_chain_status': (i32, [vp, P(C.c_uint32), vp]),
        'rlrep_build_flags': (i32, []),
        'rlrep_debug_stamp': (i32, [vp, i32, i32, vp]),
        'rlrep_history': (i32, [vp, i32]),
        'rlrep_history_dev': (i32, [vp, P(vp), P(vp), P(i32), P(i32), P(i32)]),
        'rlrep_metrics_dev': (vp, [vp]),
        'rlrep_last_launch_count': (i32, [vp]),
        'rlrep_launch_counter': (i64, []),
        'rlrep_front_end_counts': (i32, [P(i64)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)       # AttributeError if the library does not export it
        fn.restype, fn.argtypes = res, args
    if lib.rlrep_abi_version() != 4:
        raise RuntimeError('librlrep_hip.so ABI version mismatch')
    return lib, sig


lib, SIGNATURES = _load()


def has_experiments():
    """True if the loaded library carries the opt-in engines (built with RLREP_BUILD_EXPERIMENTS=1)."""
    return bool(lib.rlrep_build_flags() & 1)


def check(rc, what=''):
    if rc != 0:
        msg = lib.rlrep_last_error()
        raise RuntimeError(f'rlrep {what} failed ({rc}): {msg.decode() if msg else ""}')


def front_end_counts():
    """Launches of the 16-row tile engine per front end since the library was loaded: dict(fast, fast4, fastpre, record)."""
    out = (C.c_int64 * 4)()
    check(lib.rlrep_front_end_counts(out), 'front_end_counts')
    return dict(zip(('fast', 'fast4', 'fastpre', 'record'), (int(v) for v in out)))
