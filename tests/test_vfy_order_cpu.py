"""The order plan of mldsa_vfy_verify (fips204_amd/vfy/vfy_parts.h, order_plan) without a device: tests/cpp/vfy_order_main.cpp models
the lanes as FIFOs and the events as edges, and checks what the plan orders behind what for calls of 1, 2, 3 and 7 parts, alone and back
to back, and that no record or wait of it can go.  enqueue() (vfy.hip) walks the same list, one runtime call per step."""
import os
import re

from layer_checks import ROOT, sanitized_program

VFY_DIR = os.path.join(ROOT, "fips204_amd", "vfy")


def test_the_order_plan_under_asan_and_ubsan(tmp_path):
    sanitized_program(tmp_path, "vfy_order", ["vfy_order_main.cpp"], "vfy_order OK")


def test_enqueue_issues_the_plan_and_nothing_beside_it():
    """the plan is what runs: enqueue() takes its lanes, events and launches from order_plan(), and no other place of the library orders
    streams"""
    src = open(os.path.join(VFY_DIR, "vfy.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    body = code[code.index("int enqueue("):code.index("void drain(")]
    assert "order_plan(plan.n_parts())" in body and "for (const Step& st : order.steps)" in body
    assert body.count("hipEventRecord(") == 1 and body.count("hipStreamWaitEvent(") == 1
    assert "d->ea" not in body.replace("{s, d->ea, d->vm}", "") and "d->vm" not in body.replace("{s, d->ea, d->vm}", "")
    # outside enqueue() events are recorded by the profile scope only, and nothing else waits for one
    rest = code.replace(body, "")
    assert rest.count("hipStreamWaitEvent(") == 0 and rest.count("hipEventRecord(") == 2
    # a half-enqueued call still drains both library streams
    drain = code[code.index("void drain("):code.index("size_t scratch_bytes_of(")]
    assert "hipStreamSynchronize(d->ea)" in drain and "hipStreamSynchronize(d->vm)" in drain
