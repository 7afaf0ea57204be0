"""The call record of the cross-rank argument check (HcclAmdCheckRecord; hccl_amd/csrc/ipc_plan.cc FillCheckRecord) and
the HCCL_DFS_CONFIG grammar (HcclAmdParseDfsConfig; hccl_amd/csrc/config.cc ParseDfsConfig). Host arithmetic only.

The table is the reference's FillOpExchangeInfo / FillOpExchangeInfoWithDataDes (src/ops/op_common/op_common.cc:
1259-1322): root with the invalid rank where the operator has none, reduce op RESERVED where there is none, the count
by operator (AlltoAll: sendCount; the V operators: none, their counts differ by rank)."""
import ctypes

import pytest

import hccl_amd as H
from hccl_amd import CheckField as F
from hccl_amd import CheckOp, HcclDataType, HcclReduceOp, HcclResult, OpType, lib
from hccl_amd._lib import CHECK_NO_ROOT, CHECK_WORDS

BUF = (200 << 20) + (5 << 32)  # more than 32 bits: the buffer size takes two words
COUNT = 4099 + (3 << 32)


def record(op, root=3, red=HcclReduceOp.MAX, dt=HcclDataType.FP16, count=COUNT, buf=BUF, aiv=1, strict=1, cores=48):
    rec = H.HcclAmdCheckRecordWords()
    r = lib.HcclAmdCheckRecord(int(op), root, int(red), int(dt), count, buf, aiv, strict, cores, ctypes.byref(rec))
    return r, list(rec.w)


def fields(w):
    """The record's words as {field: value}: words 0-1 the buffer size, 7-8 the count, one word each otherwise."""
    assert len(w) == CHECK_WORDS == 11
    return {F.BUFFER_SIZE: w[0] | w[1] << 32, F.ROOT: w[2], F.OP_TYPE: w[3], F.EXECUTE_CONFIG: w[4],
            F.REDUCE_OP: w[5], F.DATA_TYPE: w[6], F.COUNT: w[7] | w[8] << 32, F.AIV_CORE_LIMIT: w[9],
            F.DETERMINISTIC: w[10]}


# operator -> (has a root, has a reduce op, carries its count)
TABLE = {
    OpType.ALLREDUCE: (False, True, True),
    OpType.REDUCE_SCATTER: (False, True, True),
    OpType.REDUCE: (True, True, True),
    OpType.ALLGATHER: (False, False, True),
    OpType.BROADCAST: (True, False, True),
    OpType.SCATTER: (True, False, True),
    OpType.ALLTOALL: (False, False, True),
    OpType.REDUCE_SCATTER_V: (False, True, False),
    OpType.ALLGATHER_V: (False, False, False),
    CheckOp.ALLTOALLV: (False, False, False),
    CheckOp.ALLTOALLVC: (False, False, False),
}


@pytest.mark.parametrize("op", list(TABLE), ids=lambda o: o.name)
def test_record_of_every_checked_operator(op):
    has_root, has_red, has_count = TABLE[op]
    r, w = record(op)
    assert r == HcclResult.HCCL_SUCCESS
    f = fields(w)
    assert f[F.OP_TYPE] == int(op)
    assert f[F.ROOT] == (3 if has_root else CHECK_NO_ROOT)
    assert f[F.REDUCE_OP] == (HcclReduceOp.MAX if has_red else HcclReduceOp.RESERVED)
    assert f[F.DATA_TYPE] == HcclDataType.FP16
    assert f[F.COUNT] == (COUNT if has_count else 0)
    assert f[F.BUFFER_SIZE] == BUF
    assert f[F.EXECUTE_CONFIG] == 1 and f[F.DETERMINISTIC] == 1 and f[F.AIV_CORE_LIMIT] == 48


def test_record_of_the_barrier_has_no_data_description():
    r, w = record(OpType.BARRIER)
    assert r == HcclResult.HCCL_SUCCESS
    f = fields(w)
    assert f[F.OP_TYPE] == OpType.BARRIER and f[F.ROOT] == CHECK_NO_ROOT
    assert f[F.REDUCE_OP] == HcclReduceOp.RESERVED and f[F.DATA_TYPE] == HcclDataType.RESERVED and f[F.COUNT] == 0


def test_v_operators_with_different_counts_have_equal_records():
    for op in (OpType.REDUCE_SCATTER_V, OpType.ALLGATHER_V, CheckOp.ALLTOALLV, CheckOp.ALLTOALLVC):
        assert record(op, count=5)[1] == record(op, count=7)[1]
    assert record(OpType.ALLTOALL, count=5)[1] != record(OpType.ALLTOALL, count=7)[1]


def test_every_field_changes_exactly_its_words():
    base = fields(record(OpType.REDUCE)[1])
    for kw, field in ((dict(root=2), F.ROOT), (dict(red=HcclReduceOp.SUM), F.REDUCE_OP),
                      (dict(dt=HcclDataType.FP32), F.DATA_TYPE), (dict(count=COUNT + 1), F.COUNT),
                      (dict(buf=BUF + (1 << 32)), F.BUFFER_SIZE), (dict(aiv=0), F.EXECUTE_CONFIG),
                      (dict(strict=0), F.DETERMINISTIC), (dict(cores=24), F.AIV_CORE_LIMIT)):
        other = fields(record(OpType.REDUCE, **kw)[1])
        assert [k for k in base if base[k] != other[k]] == [field]


def test_unchecked_operators_and_null_record():
    rec = H.HcclAmdCheckRecordWords()
    for op in (-1, 12, 100):  # send, receive and the batch have no record: they are not collective
        assert lib.HcclAmdCheckRecord(op, 0, 0, 0, 1, BUF, 0, 0, 48, ctypes.byref(rec)) == HcclResult.HCCL_E_PARA
    assert lib.HcclAmdCheckRecord(0, 0, 0, 0, 1, BUF, 0, 0, 48, None) == HcclResult.HCCL_E_PTR


def test_field_names_are_the_references():
    names = [lib.HcclAmdCheckFieldName(i) for i in range(len(F))]
    assert names == [b"HcclBufferSize", b"RootRankId", b"OpType", b"OpExecuteConfig", b"HcclReduceOp", b"HcclDataType",
                     b"DataCount", b"AivCoreLimit", b"HcclDeterministic"]
    assert lib.HcclAmdCheckFieldName(-1) is None and lib.HcclAmdCheckFieldName(len(F)) is None


def parse(text, start=-1):
    v = ctypes.c_int32(start)
    return lib.HcclAmdParseDfsConfig(text.encode(), ctypes.byref(v)), v.value


@pytest.mark.parametrize("text, want", [
    ("inconsistent_check:on", 1),
    (" Inconsistent_Check : FIRST ,task_exception:off", 0),
    ("inconsistent_check:off", -1),
    ("task_exception:on", -1),              # the switch keeps its default: unset means off here
    ("some_other_key:whatever", -1),        # unknown keys are ignored
    ("inconsistent_check:first,inconsistent_check:on", 1),
    ("   ", -1),                            # blanks only: no item
])
def test_dfs_config_grammar(text, want):
    assert parse(text) == (HcclResult.HCCL_SUCCESS, want)


@pytest.mark.parametrize("text", [
    "inconsistent_check", "inconsistent_check:", "inconsistent_check:yes", "inconsistent_check:on:off",
    "inconsistent_check:on,", ",inconsistent_check:on", "inconsistent_check:on,,task_exception:on",
    "task_exception:maybe", "inconsistent_check:on,task_exception",
])
def test_malformed_dfs_config_is_refused_and_leaves_the_switch(text):
    assert parse(text, start=-1) == (HcclResult.HCCL_E_PARA, -1)
    assert parse(text, start=0) == (HcclResult.HCCL_E_PARA, 0)


def test_off_only_overrides_an_earlier_value():
    assert parse("inconsistent_check:off", start=1) == (HcclResult.HCCL_SUCCESS, -1)


def test_config_key_is_declared():
    assert H.Config.INCONSISTENT_CHECK == 20
