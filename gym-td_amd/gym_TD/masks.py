"""Legal-action masks restated in numpy: the reference of ``TDEngine.action_mask``.

For one board's canonical state (the dict ``TDEngine.board_state`` and
``oracle.canon.oracle_state`` both produce, plus ``num_roads``), which action the next
step would execute if it were the only thing asked of that side -- the checks of
TDBoard.tower_build / tower_lvup / tower_destruct / summon_cluster (TDBoard.py:199-293)
behind the cool-down gates of TDDefense.py:38-39,64 and TDAttack.py:31-33, in their
order, with the device's two capacity rules (32 towers, 128 enemies) on request.
"""
import numpy as np

from . import fail_code as FC

TOWER_CAP, ENEMY_CAP = 32, 128
FC_CAPACITY = 6  # the device's answer to a 33rd tower (no reference counterpart)


def reference_masks(state, L, cfg, hp, mode="def", multi=False, cap=True):
    """(def_mask, def_code, atk_mask) of one board, uint8.

    state: steps, cost_def, cost_atk, attacker_cd, defender_cd, towers [(type, lv, r, c, cd)],
           enemies [...], map6 (L*L ints, row-major), num_roads.
    def_mask / def_code: (6 L^2 + 1,), or (6, L, L) with ``multi``; None in mode 'atk'.
    atk_mask: (3, 5); None in mode 'def'.
    cap: apply the device's capacity rules (the reference and the oracle have none).
    A state without a playable layout (num_roads outside 1..3: the board was never reset)
    keeps only the always-legal entries.
    """
    NC = L * L
    num_roads = int(state["num_roads"])
    live = 1 <= num_roads <= 3
    def_mask = def_code = atk_mask = None
    if mode != "atk":
        cost = state["cost_def"]
        blocked = np.asarray(state["map6"], dtype=np.int64).reshape(NC) > 0
        code = np.zeros((6, NC), dtype=np.uint8)
        full = cap and len(state["towers"]) >= TOWER_CAP
        for t in range(4):
            if cost < cfg.tower_cost[t][0]:
                code[t, :] = FC.COST_SHORTAGE
            else:
                code[t, :] = FC_CAPACITY if full else 0
                code[t, blocked] = FC.INVALID_POSITION
        code[4, :] = FC.UNKNOWN_TARGET
        code[5, :] = FC.UNKNOWN_TARGET
        for (t, lv, r, c, _cd) in state["towers"]:
            cell = r * L + c
            if lv >= cfg.max_tower_lv:
                code[4, cell] = FC.LV_MAX
            elif cost < cfg.tower_cost[t][lv + 1]:
                code[4, cell] = FC.COST_SHORTAGE
            else:
                code[4, cell] = 0
            code[5, cell] = 0
        open_ = live and state["defender_cd"] <= 1
        mask = ((code == 0) & open_).astype(np.uint8)
        if multi:
            def_mask, def_code = mask.reshape(6, L, L), code.reshape(6, L, L)
        else:
            def_mask = np.concatenate([mask.reshape(-1), np.ones(1, dtype=np.uint8)])
            def_code = np.concatenate([code.reshape(-1), np.zeros(1, dtype=np.uint8)])
    if mode != "def":
        lv = 1 if state["steps"] / hp.max_episode_steps >= cfg.enemy_upgrade_at else 0
        atk_mask = np.zeros((3, 5), dtype=np.uint8)
        atk_mask[:, 4] = 1
        open_ = live and state["attacker_cd"] <= 1 and not (cap and len(state["enemies"]) >= ENEMY_CAP)
        for road in range(min(num_roads, 3) if open_ else 0):
            for t in range(4):
                atk_mask[road, t] = 0 if state["cost_atk"] < cfg.enemy_cost[t][lv] else 1
    return def_mask, def_code, atk_mask
