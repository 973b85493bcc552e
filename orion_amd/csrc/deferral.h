// deferral.h -- where the C-ABI's deferrals are decided.  Host only: call names
// and handle numbers in, a state and an action out; no HIP, no ciphertext.
//
// Rotation: RotateNew(x, k) -> r only records the rotation (r has its level,
// scale and batch, no buffer); AddCiphertext(x, r) into the rotation's own
// source records the sum (RotationAdded); DeleteCiphertext(r) then runs the
// pair as one key switch whose store adds into x, and r is never formed (the
// frontend's `out += out.roll(k)`, linear.py:72-73).  ModDown:
// EvaluateLinearTransform and MulRelinCiphertextNew return r holding its QP
// accumulator (Ciphertext::pend) where moddown_rescale applies; Rescale /
// RescaleNew of r as the next call runs both as one division by P q_l.  Any
// other call first runs what is pending as the op-by-op calls would have;
// metadata reads and deletes of other handles keep it pending; deleting r drops
// it.  Another context that reads a pending ModDown's r runs the plain ModDown
// itself (backend.hip foreign_finish).  ORION_DEFER=0 opens nothing.
#pragma once
#include <cstring>

namespace deferral {

// One row per C-ABI call that has a property (every other call has neither);
// each entry point looks its row up once, into a function-local static.
// capture: it only enqueues device work or reads host metadata, so it may be
// recorded into an open graph capture.  keeps: it leaves pending work pending
// -- metadata reads, and the four calls that send an event of their own
// (AddCiphertext, DeleteCiphertext, Rescale, RescaleNew).
struct Call {
  const char* name;
  bool capture, keeps;
};
constexpr Call kCalls[] = {
    {"AddCiphertext", 1, 1}, {"AddCiphertextNew", 1, 0}, {"AddPlaintext", 1, 0}, {"AddPlaintextNew", 1, 0},
    {"AddScalar", 1, 0}, {"AddScalarNew", 1, 0}, {"CloneCiphertext", 1, 0}, {"DeleteCiphertext", 1, 1},
    {"DeletePlaintext", 1, 1}, {"EvaluateLinearTransform", 1, 0}, {"EvaluatePolynomial", 1, 0},
    {"GaloisElement", 1, 1}, {"GetCiphertextBatch", 1, 1}, {"GetCiphertextDegree", 1, 1},
    {"GetCiphertextLevel", 1, 1}, {"GetCiphertextScale", 1, 1}, {"GetCiphertextScaleF", 1, 1},
    {"GetCiphertextSlots", 1, 1}, {"GetLiveCiphertexts", 1, 1}, {"GetLivePlaintexts", 1, 1},
    {"GetModuliChain", 1, 1}, {"GetPlaintextBatch", 1, 1}, {"GetPlaintextLevel", 1, 1},
    {"GetPlaintextScale", 1, 1}, {"GetPlaintextSlots", 1, 1}, {"ModDropCiphertext", 1, 0},
    {"MulPlaintext", 1, 0}, {"MulPlaintextNew", 1, 0}, {"MulRelinCiphertext", 1, 0},
    {"MulRelinCiphertextNew", 1, 0}, {"MulScalarFloat", 1, 0}, {"MulScalarFloatNew", 1, 0},
    {"MulScalarInt", 1, 0}, {"MulScalarIntNew", 1, 0}, {"Negate", 1, 0}, {"OrionHipConjugateNew", 1, 0},
    {"OrionHipCurrentPipeline", 1, 1},
    {"OrionHipEvaluateLinearTransformBlocks", 1, 0}, {"OrionHipGetStream", 1, 1}, {"OrionHipGraphEnd", 1, 0},
    {"OrionHipMulRelinSum", 1, 0}, {"OrionHipPackComplex", 1, 0}, {"OrionHipPackMonomials", 1, 0},
    {"OrionHipPeerCount", 0, 1},
    {"OrionHipPeerSelect", 0, 1}, {"OrionHipRotateAdd", 1, 0}, {"OrionHipRotateHoisted", 1, 0},
    {"OrionHipRotateSum", 1, 0}, {"OrionHipSlotTraceNew", 1, 0}, {"OrionHipUnpackComplex", 1, 0},
    {"OrionHipUnpackMonomials", 1, 0}, {"Rescale", 1, 1},
    {"RescaleNew", 1, 1},
    {"Rotate", 1, 0}, {"RotateNew", 1, 0}, {"SetCiphertextScale", 1, 0}, {"SetPlaintextScale", 1, 0},
    {"SubCiphertext", 1, 0}, {"SubCiphertextNew", 1, 0}, {"SubPlaintext", 1, 0}, {"SubPlaintextNew", 1, 0},
    {"SubScalar", 1, 0}, {"SubScalarNew", 1, 0}};
inline Call call(const char* name) {
  for (const Call& c : kCalls)
    if (!strcmp(c.name, name)) return c;
  return Call{name, false, false};
}

enum class Kind { None, Rotation, RotationAdded, ModDown };
struct Pending {
  Kind kind = Kind::None;
  int x = -1, r = -1, k = 0;  // r = Rotate(x, k); ModDown: r alone
};
// Keeps / Flushes: any call by its row; Add(a, b), Delete(a), Rescale(a): the
// call's handles; OpenRotation(a = x, b = r, k), OpenModDown(a = r): the call
// (which has flushed as any other) returned r with its work pending
enum class Ev { Keeps, Flushes, Add, Delete, Rescale, OpenRotation, OpenModDown };
struct Event {
  Ev ev;
  int a = -1, b = -1, k = 0;
};
// Before the state changes, RecordAdd checks that x may be written in place and
// ModDownRescale that r may; a refusal leaves the work pending.  Where another
// context has run the ModDown meanwhile, ModDownRescale has nothing to run.
enum class Act { None, Rotate, RotateThenAdd, FusedRotateAdd, DropRotation, ModDown, ModDownRescale, DropModDown,
                 RecordAdd };
struct Step {
  Pending next;
  Act act;
};

inline Step step(const Pending& p, const Event& e) {
  if (e.ev == Ev::OpenRotation) return {{Kind::Rotation, e.a, e.b, e.k}, Act::None};
  if (e.ev == Ev::OpenModDown) return {{Kind::ModDown, -1, e.a, 0}, Act::None};
  if (p.kind == Kind::None || e.ev == Ev::Keeps) return {p, Act::None};
  const bool md = p.kind == Kind::ModDown, added = p.kind == Kind::RotationAdded;
  if (e.ev == Ev::Add && p.kind == Kind::Rotation && e.a == p.x && e.b == p.r)
    return {{Kind::RotationAdded, p.x, p.r, p.k}, Act::RecordAdd};
  if (e.ev == Ev::Rescale && md && e.a == p.r) return {{}, Act::ModDownRescale};
  if (e.ev == Ev::Delete) {
    // r dies unread: a bare rotation or a ModDown never runs
    if (e.a == p.r) return {{}, md ? Act::DropModDown : added ? Act::FusedRotateAdd : Act::DropRotation};
    if (md || e.a != p.x) return {p, Act::None};
  }
  return {{}, md ? Act::ModDown : added ? Act::RotateThenAdd : Act::Rotate};  // the flush
}

}  // namespace deferral
