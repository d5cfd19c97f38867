"""A literal Python transcription of the open_karto members behind the scan-intake stage, member by member, for the
tests: none of the batch or wave formulations of include/slam2d/karto_process.h appears here.

  LaserRangeFinder.get_offset_pose     the identity offset every Karto header of this library assumes
  LocalizedRangeScan                   Karto.h:5225-5313: Set/GetCorrectedPose, GetSensorPose, SetSensorPose, GetSensorAt
  ScanManager.add_running_scan         Mapper.h:1365-1386, a real list and the while loop as written
  Mapper.has_moved_enough              Mapper.cpp:2087-2120
  Mapper.process                       Mapper.cpp:1999-2079 with one sensor; the matcher, the graph and the loop closure
                                       are callbacks (the worlds of karto_process_cases.py give their results)
  SlamKarto.add_scan                   karto_slam.cc:415-440: the readings loop with its reversal, the two SetPose calls

Pose2, Matrix3, Transform and normalize_angle are karto_link_plain's; sin / cos / atan2 are the restatement's exported
detmath wrappers (the only arithmetic not Python's own).  Test infrastructure: nothing here is imported by the package.
"""
from __future__ import annotations

import math

import numpy as np

import karto_link_plain as P
import karto_link_ref as LR
import karto_process_ref as R
from karto_link_plain import KT_TOLERANCE, Pose2, Transform, normalize_angle


def square(v):  # math::Square
    return v * v


def squared_distance(a: Pose2, b: Pose2) -> float:
    """Pose2::SquaredDistance = Vector2::SquaredDistance: (*this - rOther).SquaredLength()."""
    dx, dy = a.x - b.x, a.y - b.y
    return square(dx) + square(dy)


class LaserRangeFinder:
    def get_offset_pose(self) -> Pose2:
        return Pose2()


class LocalizedRangeScan:
    def __init__(self, laser: LaserRangeFinder, readings):
        self.laser, self.readings = laser, readings
        self.odometric_pose, self.corrected_pose = Pose2(), Pose2()
        self.time = 0.0
        self.state_id = -1

    def set_odometric_pose(self, pose: Pose2):
        self.odometric_pose = Pose2(*pose.tolist())

    def set_corrected_pose(self, pose: Pose2):
        self.corrected_pose = Pose2(*pose.tolist())

    def get_sensor_at(self, rPose: Pose2) -> Pose2:
        return Transform(Pose2(), rPose).transform_pose(self.laser.get_offset_pose())

    def get_sensor_pose(self) -> Pose2:
        return self.get_sensor_at(self.corrected_pose)

    def set_sensor_pose(self, rScanPose: Pose2):
        deviceOffsetPose2 = self.laser.get_offset_pose()
        offsetLength = math.sqrt(square(deviceOffsetPose2.x) + square(deviceOffsetPose2.y))
        offsetHeading = deviceOffsetPose2.heading
        angleoffset = LR.atan2(deviceOffsetPose2.y, deviceOffsetPose2.x)
        correctedHeading = normalize_angle(rScanPose.heading)
        worldSensorOffset = Pose2(offsetLength * LR.cos(correctedHeading + angleoffset - offsetHeading),
                                  offsetLength * LR.sin(correctedHeading + angleoffset - offsetHeading), offsetHeading)
        self.corrected_pose = rScanPose - worldSensorOffset


class ScanManager:
    def __init__(self, running_buffer_maximum_size: int, running_buffer_maximum_distance: float):
        self.scans, self.running_scans, self.last_scan = [], [], None
        self.max_size, self.max_distance = running_buffer_maximum_size, running_buffer_maximum_distance

    def add_scan(self, scan):
        scan.state_id = len(self.scans)
        self.scans.append(scan)

    def add_running_scan(self, pScan):
        self.running_scans.append(pScan)
        frontScanPose = self.running_scans[0].get_sensor_pose()
        backScanPose = self.running_scans[-1].get_sensor_pose()
        squaredDistance = squared_distance(frontScanPose, backScanPose)
        while (len(self.running_scans) > self.max_size or
               squaredDistance > square(self.max_distance) - KT_TOLERANCE):
            del self.running_scans[0]
            frontScanPose = self.running_scans[0].get_sensor_pose()
            backScanPose = self.running_scans[-1].get_sensor_pose()
            squaredDistance = squared_distance(frontScanPose, backScanPose)


class Mapper:
    def __init__(self, params: dict):
        self.p = params
        self.manager = ScanManager(int(params["scan_buffer_size"]), float(params["scan_buffer_maximum_scan_distance"]))

    def has_moved_enough(self, pScan, pLastScan) -> bool:
        if pLastScan is None:
            return True
        timeInterval = pScan.time - pLastScan.time
        if timeInterval >= self.p["minimum_time_interval"]:
            return True
        lastScannerPose = pLastScan.get_sensor_at(pLastScan.odometric_pose)
        scannerPose = pScan.get_sensor_at(pScan.odometric_pose)
        deltaHeading = normalize_angle(scannerPose.heading - lastScannerPose.heading)
        if abs(deltaHeading) >= self.p["minimum_travel_heading"]:
            return True
        squaredTravelDistance = squared_distance(lastScannerPose, scannerPose)
        if squaredTravelDistance >= square(self.p["minimum_travel_distance"]) - KT_TOLERANCE:
            return True
        return False

    def process(self, pScan, match_scan=None, add_vertex=None, add_edges=None, try_close_loop=None, stop_after_gate=False):
        """Mapper::Process.  match_scan(scan, running scans) -> bestPose or None (the matcher threw: the pose stays);
        add_vertex(scan), add_edges(scan), try_close_loop(scan) may move the scan through set_sensor_pose."""
        pLastScan = self.manager.last_scan
        if pLastScan is not None:
            lastTransform = Transform(pLastScan.odometric_pose, pLastScan.corrected_pose)
            pScan.set_corrected_pose(lastTransform.transform_pose(pScan.odometric_pose))
        if not self.has_moved_enough(pScan, pLastScan):
            return False
        if stop_after_gate:
            return True
        if pLastScan is not None and match_scan is not None:
            bestPose = match_scan(pScan, self.manager.running_scans)
            if bestPose is not None:
                pScan.set_sensor_pose(bestPose)
        self.manager.add_scan(pScan)
        if add_vertex is not None:
            add_vertex(pScan)
        if add_edges is not None:
            add_edges(pScan)
        self.manager.add_running_scan(pScan)
        if try_close_loop is not None:
            try_close_loop(pScan)
        self.manager.last_scan = pScan
        return True


class SlamKarto:
    def __init__(self, inverted: bool):
        self.laser, self.inverted = LaserRangeFinder(), bool(inverted)

    def add_scan(self, ranges, time: float, karto_pose: Pose2) -> LocalizedRangeScan:
        """addScan up to mapper_->Process: ranges is the LaserScan's float array."""
        readings = []
        if self.inverted:
            for it in reversed(list(ranges)):
                readings.append(float(it))
        else:
            for it in list(ranges):
                readings.append(float(it))
        range_scan = LocalizedRangeScan(self.laser, readings)
        range_scan.time = float(time)
        range_scan.set_odometric_pose(karto_pose)
        range_scan.set_corrected_pose(karto_pose)
        return range_scan


# ------------------------------------------------------------------------------------------------ worlds
def graph_of(w: dict, g: int, pool_poses, states=None):
    """Graph g of a world as reference objects: a Mapper whose manager holds the graph's scans at their current pool
    poses (SetSensorPose), the running scans and the last scan with its odometric pose and time."""
    st = (w["states"] if states is None else states)[g]
    off = int(w["pool_offset"][g])
    node = SlamKarto(w["params"]["inverted"])
    m = Mapper(w["params"])
    for i in range(int(st["n_scans"])):
        s = LocalizedRangeScan(node.laser, None)
        if off + i < len(pool_poses):
            s.set_sensor_pose(Pose2(*pool_poses[off + i]))
        m.manager.add_scan(s)
    b, n = int(st["run_begin"]), int(st["run_length"])
    m.manager.running_scans = m.manager.scans[b:b + n]
    if m.manager.scans:
        last = m.manager.scans[-1]
        last.set_odometric_pose(Pose2(*st["last_odom"]))
        last.time = float(st["last_time"])
        m.manager.last_scan = last
    return node, m


def intake(w: dict) -> dict:
    """What kp_intake_device must give for a world, from Mapper.process up to the gate per candidate; the library's
    own rules (an absent row, a full graph, a slot out of range) are applied around it."""
    o = R.empty_outputs(w)
    nr, g_first = int(w["n_readings"]), int(w.get("g_first", 0))
    pool_scans = len(o["pool_poses"])
    before = np.array(w["pool_poses"], np.float64)
    query, base_begin, base_index, n_jobs = [], [0], [], 0
    for i, c in enumerate(w["cand"]):
        g = g_first + i
        st, off = w["states"][g], int(w["pool_offset"][g])
        r = o["rec"][i]
        r["status"], r["accepted"], r["match_status"], r["pad_"] = R.KP_OK, 0, 0, 0
        r["scan"] = r["prev"] = r["job"] = r["seq"] = -1
        r["run_begin"], r["run_length"] = st["run_begin"], st["run_length"]
        r["corrected"] = r["sensor"] = 0.0
        row, n_scans = int(c["row"]), int(st["n_scans"])
        if row < 0:
            continue
        if row >= len(w["ranges_f32"]):
            r["status"] = R.KP_EINVAL
            continue
        if n_scans > 0:
            r["prev"] = n_scans - 1
            if off + n_scans - 1 >= pool_scans:
                r["status"] = R.KP_EINVAL
                continue
        node, mapper = graph_of(w, g, before)
        scan = node.add_scan(w["ranges_f32"][row], c["time"], Pose2(*c["odom"]))
        moved = mapper.process(scan, stop_after_gate=True)
        r["corrected"] = scan.corrected_pose.tolist()
        r["sensor"] = scan.get_sensor_pose().tolist()
        if not moved:
            continue
        if n_scans >= int(w["max_scans"]):
            r["status"] = R.KP_ERANGE
            continue
        if off + n_scans >= pool_scans:
            r["status"] = R.KP_EINVAL
            continue
        r["accepted"], r["scan"], r["job"] = 1, n_scans, n_jobs
        o["pool_ranges"][off + n_scans] = scan.readings
        o["pool_poses"][off + n_scans] = scan.get_sensor_pose().tolist()
        seq = -1
        if mapper.manager.last_scan is not None:
            seq = len(query)
            query.append(off + n_scans)
            base_index += [off + s.state_id for s in mapper.manager.running_scans]
            base_begin.append(len(base_index))
            o["items"][seq] = (g, n_scans, st["run_begin"], st["run_length"])
        r["seq"] = seq
        o["jobs"][n_jobs] = (g, n_scans, off, n_scans - 1 if n_scans else -1, seq, seq, 0, 0)
        o["queries"][n_jobs] = (g, n_scans, 0, -1, -1)
        n_jobs += 1
    o["query"][:len(query)] = query
    o["base_begin"][:len(base_begin)] = base_begin
    o["base_index"][:len(base_index)] = base_index
    o["n_seq"][0], o["n_jobs"][0] = len(query), n_jobs
    return o


def apply(w: dict, rec, seq, pool_poses):
    """pScan->SetSensorPose(bestPose) and the pose AddNode reads."""
    rec, pool = np.array(rec, R.INTAKE, copy=True), np.array(pool_poses, np.float64, copy=True)
    node = SlamKarto(w["params"]["inverted"])
    for i, r in enumerate(rec):
        if not r["accepted"] or r["seq"] < 0:
            continue
        if r["seq"] >= len(seq):
            r["match_status"] = R.KP_EINVAL
            continue
        m = seq[int(r["seq"])]
        r["match_status"] = m["status"]
        if m["status"] != R.KT_OK:  # the matcher threw: Process does not get to SetSensorPose
            continue
        scan = LocalizedRangeScan(node.laser, None)
        scan.set_sensor_pose(Pose2(*m["mean"]))
        r["sensor"], r["corrected"] = m["mean"], scan.corrected_pose.tolist()
        pool[int(w["pool_offset"][int(w.get("g_first", 0)) + i]) + int(r["scan"])] = m["mean"]
    return rec, pool


def bind_near(jobs, n_jobs: int, source, n_matches: int):
    jobs = np.array(jobs, R.JOB, copy=True)
    for j in range(n_jobs):
        mine = [m for m in range(n_matches) if int(source[m]["slot"]) == j]
        first = mine[0] if mine else sum(1 for m in range(n_matches) if int(source[m]["slot"]) < j)
        jobs[j]["near_first"], jobs[j]["near_count"] = first, len(mine)
    return jobs


def advance(w: dict, rec, pool_poses, states=None):
    """AddRunningScan and SetLastScan per accepted candidate, at the current pool poses."""
    st = np.array(w["states"] if states is None else states, R.STATE, copy=True)
    adv = R.poisoned(len(rec), R.ADVANCED)
    g_first = int(w.get("g_first", 0))
    for i, r in enumerate(rec):
        g = g_first + i
        a = adv[i]
        a["accepted"], a["corrected"] = 0, 0.0
        if r["accepted"]:
            node, mapper = graph_of(w, g, pool_poses, st)
            scan = LocalizedRangeScan(node.laser, None)
            scan.set_sensor_pose(Pose2(*pool_poses[int(w["pool_offset"][g]) + int(r["scan"])]))
            mapper.manager.add_scan(scan)
            assert scan.state_id == int(r["scan"])
            mapper.manager.add_running_scan(scan)
            run = mapper.manager.running_scans
            st[g]["run_begin"], st[g]["run_length"] = run[0].state_id, len(run)
            assert [s.state_id for s in run] == list(range(run[0].state_id, run[0].state_id + len(run)))
            st[g]["n_scans"] = len(mapper.manager.scans)
            st[g]["last_time"], st[g]["last_odom"] = w["cand"][i]["time"], w["cand"][i]["odom"]  # SetLastScan
            a["accepted"], a["corrected"] = 1, scan.corrected_pose.tolist()
        a["run_begin"], a["run_length"], a["n_scans"] = st[g]["run_begin"], st[g]["run_length"], st[g]["n_scans"]
    return adv, st
